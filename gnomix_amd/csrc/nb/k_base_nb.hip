// k_base_nb.hip — the three Naive-Bayes bases (NBBernoulliBase, NBMultinomialBase, NBGaussianBase) on gfx950: one likelihood-table
// kernel on the float64 matrix cores, the model load behind gnx_model_load_nb, and the counting kernel of the fit.
//
// Replaces NB*Base.predict_proba (reference src/Base/models.py:96-132 through src/Base/base.py:146-180): per window
//   sklearn BernoulliNB(alpha=0) / MultinomialNB(alpha=0) / GaussianNB() .predict_proba(Xw).
//
// Semantics, complete:
//  * On SNP codes x in {0, 1, 2, 3} all three classifiers have one form.  For query haplotype n and window w
//      jll[n, c] = bias[w, c] + sum_p T[w, p, x[n, col(w, p)], c]      p = 0 .. width_w - 1, IN THIS ORDER
//      B[n, w, :] = softmax_c(jll)
//    col(w, p) is the window's slice of the reflect-padded query (base.py:41-44; width M + 2 ctx, the last window + rem).  The sum
//    is a plain sequential float64 sum that starts at bias: one rounding per position (see "Arithmetic").
//  * T and bias are built by the caller from the fitted attributes (gnomix_amd.convert.nb_window_from_sklearn), class column
//    c = classes_[k], flp = feature_log_prob_:
//      Bernoulli (binarize = 0):  T[p,0,c] = log(1 - exp(flp[c,p])),  T[p,v>=1,c] = flp[c,p];   bias = class_log_prior_
//      Multinomial:               T[p,v,c] = v * flp[c,p];                                      bias = class_log_prior_
//      Gaussian:                  T[p,v,c] = -0.5 (v - theta_[c,p])^2 / var_[c,p];
//                                 bias[c] = log(class_prior_[c]) - 0.5 sum_p log(2 pi var_[c,p])
//  * Codes are numbers: 2 = missing is the number 2.  A query code 3 (the largest a 2-bit packed row can hold) reads table row 3:
//    the number 3 for Multinomial and Gaussian, "non-zero" for Bernoulli.  Other int8 values are outside the contract; the kernel
//    uses their two low bits, so nothing is read out of bounds.
//  * A class absent from a window's classes_ has bias = -inf: its table rows are taken as zero and its output column is exactly 0.
//    -inf is allowed only in bias, and at least one class per window must be present.  Absent classes never enter the matrix
//    pipe as infinities: load turns them into a per-window mask of present columns.
//  * Normalisation: m = max_c jll over the present classes; e_c = exp(jll_c - m) (gnx_exp.h; the argument is floored at -746, where
//    float64 exp is already 0); B_c = e_c * (1 / sum_c e_c), one reciprocal per row (gnx_rcp_nr).  The largest class has e = 1
//    exactly, so the sum is in [1, 16].
//  * The float32 output is the float32 rounding of the float64 output.  A <= 16 (one column tile); A > 16 is GNX_EUNSUPPORTED.
//  * Refused at load (GNX_EINVAL): a non-finite table entry (0 * inf would be NaN in the matrix pipe; the message names the window),
//    NaN or +inf in bias, a window with no class present, a width that is not the window's width.
//
// Arithmetic.  v_mfma_f64_16x16x4_f64 has K = 4, and K = 4 is the four codes: for 16 query rows and one SNP position p the A operand
// of lane l is (x[row = l & 15][p] == (l >> 4)) ? 1.0 : 0.0 and the B operand is T[p][l >> 4][l & 15].  Three of the four products
// are exact zeros and the fourth is T[p][x][c] itself, so the accumulator after position p is fl(acc + T[p][x][c]): the sequential
// sum above, whichever way the instruction orders or fuses its four terms.  The tables sit in HBM as (position, 4, 16) doubles
// (columns >= A and absent classes zero), which IS the B-operand stream: one coalesced 512-byte load per position.
// Layout:
//  * a block = one window x NB_ROWS query rows, 4 waves; a wave keeps NB_MT 16-row tiles' accumulators (4 float64 each) in registers
//    and reuses every loaded B operand across them (the other three waves' loads of the same 512 bytes hit the cache);
//  * a lane reads its row's window bytes 16 at a time (one unaligned 16-byte load per 16 positions; the four lanes of a row read
//    the same bytes); a window that lies inside the unpadded row is a contiguous slice, only windows that touch the reflected edges
//    (the first and the last when ctx > 0) and the tail of a width that is no multiple of 16 gather byte by byte through the
//    reflected index map.  Position order is the same in every case;
//  * the epilogue stays in the accumulator layout (column = lane & 15, row = (lane >> 4) + 4 * reg): the row maximum and the row sum
//    are butterflies over the 16 lanes of a row; no LDS, no scratch, no runtime-indexed register array, plain vector stores.
//
// The fit (gnx_train_nb_counts): every fitted attribute of the three estimators is a closed form of integer counts, so the device
// counts and the host finishes in float64 with scikit-learn's own expressions (gnomix_amd.train.train_nb_base).  k_nb_count: one
// thread per (window, position) walks the fit rows; X reads are coalesced across positions, y[n, w] is the same for the whole block;
// each thread keeps its counters n1[c], n2[c] in LDS, thread-minor (no bank conflicts, no atomics).  k_nb_class_count: one thread per
// window.
#include "../gnx_internal.h"
#include "../gnx_exp.h"
#include "../gnx_window.h"

#include <cmath>
#include <cstring>

struct NbWinDev {
  int64_t tab_off;   // positions: this window's table rows start at tab[tab_off * 64]
  int32_t width;     // SNPs
  uint32_t present;  // bit c: class c is present (c < A)
};

struct NbModel {
  const NbWinDev* win = nullptr;
  const double* tab = nullptr;   // [sum of widths][4 codes][16 columns]
  const double* bias = nullptr;  // [W][16], 0 where absent or >= A
};

struct NbLaunch {
  const int8_t* X;
  int64_t N, ldx, C, ctx, M;
  int32_t W, A, w_first;
  const NbWinDev* win;
  const double* tab;
  const double* bias;
  float* b32;
  double* b64;
};

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(1))) xbytes16 { uint32_t v[4]; };

constexpr int NB_MT = 4;                  // 16-row tiles per wave
constexpr int NB_WAVES = 4;
constexpr int NB_ROWS = NB_WAVES * NB_MT * 16;  // query rows per block
constexpr int NB_PC = 16;                 // positions per X chunk (one 16-byte load per lane)

__device__ __forceinline__ xbytes16 load_x16(const int8_t* p) {  // unaligned global_load_dwordx4
  xbytes16 r;
  __builtin_memcpy(&r, p, 16);
  return r;
}

// positions p0 .. p0 + 15 of the window (those below width; the rest read as code 0 and are never used) through the index map
__device__ __forceinline__ xbytes16 gather_x16(const int8_t* row, int64_t s, int p0, int width, int64_t C, int64_t ctx) {
  xbytes16 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (p0 + 4 * q + b < width) v |= (uint32_t)(uint8_t)row[gnx_pad_src(s + p0 + 4 * q + b, C, ctx)] << (8 * b);
    r.v[q] = v;
  }
  return r;
}

// one chunk: positions p0 .. p0 + nv - 1 (nv = 16 when FULL), in order; tp = the chunk's first table row, this lane's element
template <bool FULL>
__device__ __forceinline__ void nb_chunk(d4 (&acc)[NB_MT], const xbytes16 (&x)[NB_MT], const double* tp, int nv, uint32_t kq) {
#pragma unroll
  for (int t = 0; t < NB_PC; ++t) {
    if (FULL || t < nv) {  // nv is wave-uniform
      const double b = tp[(size_t)t * 64];
#pragma unroll
      for (int mt = 0; mt < NB_MT; ++mt) {
        const uint32_t code = (x[mt].v[t >> 2] >> (8 * (t & 3))) & 3u;
        const double a = code == kq ? 1.0 : 0.0;
        acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[mt], 0, 0, 0);
      }
    }
  }
}

__global__ __launch_bounds__(NB_WAVES * 64) void k_nb_table(NbLaunch L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15;
  const uint32_t kq = (uint32_t)lane >> 4;
  const int w = L.w_first + blockIdx.y;
  const int64_t n0 = ((int64_t)blockIdx.x * NB_WAVES + wave) * (NB_MT * 16);
  if (n0 >= L.N) return;  // (no block-wide barrier below)
  const NbWinDev wd = L.win[w];
  const int width = wd.width;
  const int64_t s = (int64_t)w * L.M;  // the window's first position in the reflect-padded row
  const bool contiguous = s >= L.ctx && s + width <= L.ctx + L.C;

  const int8_t* xrow[NB_MT];
#pragma unroll
  for (int mt = 0; mt < NB_MT; ++mt) {
    const int64_t n = n0 + mt * 16 + i16;  // rows past the batch repeat the last one (never written out)
    xrow[mt] = L.X + (n < L.N ? n : L.N - 1) * L.ldx;
  }

  const bool here = i16 < L.A && ((wd.present >> i16) & 1u);
  const double bias = L.bias[(size_t)w * 16 + i16];
  d4 acc[NB_MT];
#pragma unroll
  for (int mt = 0; mt < NB_MT; ++mt) acc[mt] = d4{bias, bias, bias, bias};

  const double* tp = L.tab + (size_t)wd.tab_off * 64 + lane;
  const int n_full = contiguous ? width / NB_PC : 0;  // chunks served by 16-byte loads: every byte lies inside the row
  int p0 = 0;
  if (n_full > 0) {
    const int64_t c0 = s - L.ctx;
    xbytes16 xn[NB_MT];
#pragma unroll
    for (int mt = 0; mt < NB_MT; ++mt) xn[mt] = load_x16(xrow[mt] + c0);
    for (int c = 0; c < n_full; ++c, p0 += NB_PC) {
      xbytes16 x[NB_MT];
#pragma unroll
      for (int mt = 0; mt < NB_MT; ++mt) x[mt] = xn[mt];
      if (c + 1 < n_full) {
#pragma unroll
        for (int mt = 0; mt < NB_MT; ++mt) xn[mt] = load_x16(xrow[mt] + c0 + p0 + NB_PC);
      }
      nb_chunk<true>(acc, x, tp + (size_t)p0 * 64, NB_PC, kq);
    }
  }
  for (; p0 < width; p0 += NB_PC) {  // reflected windows, and the tail of a contiguous one
    xbytes16 x[NB_MT];
#pragma unroll
    for (int mt = 0; mt < NB_MT; ++mt) x[mt] = gather_x16(xrow[mt], s, p0, width, L.C, L.ctx);
    const int nv = width - p0 < NB_PC ? width - p0 : NB_PC;
    nb_chunk<false>(acc, x, tp + (size_t)p0 * 64, nv, kq);
  }

  // ---- softmax in the accumulator layout: column = lane & 15, row = (lane >> 4) + 4 * reg ----
#pragma unroll
  for (int mt = 0; mt < NB_MT; ++mt) {
    double m[4], e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[r] = here ? acc[mt][r] : -INFINITY;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m[r] = __builtin_fmax(m[r], __shfl_xor(m[r], o, 64));
      e[r] = here ? __builtin_fmax(acc[mt][r] - m[r], -746.0) : 0.0;
    }
    gnx_exp_scN<4>(e);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      e[r] = here ? e[r] : 0.0;
      double sum = e[r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      const double v = e[r] * gnx_rcp_nr(sum);
      const int64_t n = n0 + mt * 16 + (int)kq + 4 * r;
      if (n < L.N && i16 < L.A) {
        const size_t o = ((size_t)n * L.W + w) * L.A + i16;
        if (L.b64) L.b64[o] = v;
        if (L.b32) L.b32[o] = (float)v;
      }
    }
  }
}

// ---- the fit's counts ----
constexpr int NBC_BLOCK = 256;

__global__ __launch_bounds__(NBC_BLOCK) void k_nb_count(const int8_t* __restrict__ X, int64_t N, int64_t ldx, const int32_t* __restrict__ Y,
                                                        int64_t C, int64_t M, int64_t ctx, int32_t W, int32_t A, int32_t ldw,
                                                        int32_t w_first, int32_t* __restrict__ n1, int32_t* __restrict__ n2) {
  extern __shared__ int32_t cnt[];  // [2][A][NBC_BLOCK]: n1 then n2, thread-minor
  const int t = threadIdx.x;
  const int w = w_first + blockIdx.y;
  const int p = blockIdx.x * NBC_BLOCK + t;
  const int width = (int)(M + 2 * ctx + (w == W - 1 ? C - M * W : 0));
  for (int c = 0; c < 2 * A; ++c) cnt[c * NBC_BLOCK + t] = 0;
  if (p < width) {
    const int8_t* col = X + gnx_pad_src((int64_t)w * M + p, C, ctx);
    for (int64_t n = 0; n < N; ++n) {
      const int32_t y = Y[n * W + w];  // the same address for the whole block
      const int x = col[n * ldx];
      if ((uint32_t)y < (uint32_t)A && (x == 1 || x == 2)) cnt[((x - 1) * A + y) * NBC_BLOCK + t] += 1;
    }
  }
  if (p < ldw)
    for (int c = 0; c < A; ++c) {
      const size_t o = ((size_t)w * A + c) * ldw + p;
      n1[o] = cnt[c * NBC_BLOCK + t];
      n2[o] = cnt[(A + c) * NBC_BLOCK + t];
    }
}

__global__ __launch_bounds__(64) void k_nb_class_count(const int32_t* __restrict__ Y, int64_t N, int32_t W, int32_t A, int32_t* __restrict__ cc) {
  extern __shared__ int32_t cnt[];  // [A][64], thread-minor
  const int t = threadIdx.x;
  const int w = blockIdx.x * 64 + t;
  for (int c = 0; c < A; ++c) cnt[c * 64 + t] = 0;
  if (w < W) {
    for (int64_t n = 0; n < N; ++n) {
      const int32_t y = Y[n * W + w];
      if ((uint32_t)y < (uint32_t)A) cnt[y * 64 + t] += 1;
    }
    for (int c = 0; c < A; ++c) cc[(size_t)w * A + c] = cnt[c * 64 + t];
  }
}

hipError_t nb_counts_run(const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx, int32_t A,
                         int32_t* n1, int32_t* n2, int32_t* cc, hipStream_t s) {
  const int32_t W = (int32_t)(C / M);
  const int32_t ldw = (int32_t)(M + 2 * cx + (C - M * W));
  for (int w0 = 0; w0 < W; w0 += 32768) {
    const dim3 grid((unsigned)((ldw + NBC_BLOCK - 1) / NBC_BLOCK), (unsigned)std::min(32768, W - w0));
    hipLaunchKernelGGL(k_nb_count, grid, dim3(NBC_BLOCK), (size_t)2 * A * NBC_BLOCK * 4, s, dX, N, ldx, dy, C, M, cx, W, A, ldw, w0, n1, n2);
  }
  hipLaunchKernelGGL(k_nb_class_count, dim3((unsigned)((W + 63) / 64)), dim3(64), (size_t)A * 64 * 4, s, dy, N, W, A, cc);
  return hipGetLastError();
}

int nb_counts_check(gnx_ctx* ctx, const void* X, const void* y, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t cx, int32_t A,
                    const void* n1, const void* n2, const void* cc) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (!X || !y || !n1 || !n2 || !cc) return gnx_fail(ctx, GNX_EINVAL, "train_nb_counts: NULL pointer");
  if (A < 2 || A > 32) return gnx_fail(ctx, GNX_EINVAL, "train_nb_counts: A must be in [2, 32]");
  if (M <= 0 || C < M || cx < 0 || cx > C || C > ((int64_t)1 << 30)) return gnx_fail(ctx, GNX_EINVAL, "train_nb_counts: bad C / M / ctx");
  if (N < 1 || N >= ((int64_t)1 << 31) || ldx < C) return gnx_fail(ctx, GNX_EINVAL, "train_nb_counts: bad N / ldx");
  return GNX_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// model preparation: tables in B-operand order, bias and the mask of present classes
// ------------------------------------------------------------------------------------------------
static int nb_build(gnx_model* m, const gnx_nb_window* nb) {
  gnx_ctx* ctx = m->ctx;
  const int A = m->info.A;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W, rem = C - M * W, M_ = M + 2 * m->info.ctx;
  if (A > 16) return gnx_fail(ctx, GNX_EUNSUPPORTED, "nb base: more than 16 classes (the class columns are one 16-wide MFMA tile)");
  std::vector<NbWinDev> wins((size_t)W);
  int64_t rows = 0;
  for (int64_t i = 0; i < W; ++i) {
    const std::string wn = "nb base: window " + std::to_string(i) + ": ";
    const int64_t width = (i == W - 1) ? M_ + rem : M_;
    if (nb[i].width != width) return gnx_fail(ctx, GNX_EINVAL, wn + "nb[i].width != window width (M+2ctx, +rem for the last)");
    if (!nb[i].table || !nb[i].bias) return gnx_fail(ctx, GNX_EINVAL, wn + "table / bias is NULL");
    uint32_t present = 0;
    for (int c = 0; c < A; ++c) {
      const double b = nb[i].bias[c];
      if (std::isnan(b) || (std::isinf(b) && b > 0)) return gnx_fail(ctx, GNX_EINVAL, wn + "bias of class " + std::to_string(c) + " is NaN or +inf");
      if (!std::isinf(b)) present |= 1u << c;
    }
    if (!present) return gnx_fail(ctx, GNX_EINVAL, wn + "no class is present (every bias is -inf)");
    const double* t = nb[i].table;
    for (int64_t k = 0; k < width * 4 * A; ++k)
      if (!std::isfinite(t[k]))
        return gnx_fail(ctx, GNX_EINVAL, wn + "table entry at position " + std::to_string(k / (4 * A)) + ", code " + std::to_string(k / A % 4) +
                                             ", class " + std::to_string(k % A) + " is not finite");
    wins[(size_t)i] = NbWinDev{rows, (int32_t)width, present};
    rows += width;
  }
  std::vector<double> tab((size_t)rows * 64, 0.0), bias((size_t)W * 16, 0.0);
  for (int64_t i = 0; i < W; ++i) {
    const NbWinDev& wd = wins[(size_t)i];
    for (int c = 0; c < A; ++c) {
      if (!((wd.present >> c) & 1u)) continue;
      bias[(size_t)i * 16 + c] = nb[i].bias[c];
      for (int64_t p = 0; p < wd.width; ++p)
        for (int v = 0; v < 4; ++v) tab[((size_t)(wd.tab_off + p) * 4 + v) * 16 + c] = nb[i].table[((size_t)p * 4 + v) * A + c];
    }
  }
  auto md = std::make_shared<NbModel>();
  int rc;
  if ((rc = gnx_dev_upload(m, wins, &md->win)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, tab, &md->tab)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, bias, &md->bias)) != GNX_OK) return rc;
  m->nb = md;
  return GNX_OK;
}

int gnx_base_predict_nb(gnx_model* m, const int8_t* dX, int64_t N, int64_t ldx, float* d_b32, double* d_b64) {
  gnx_ctx* ctx = m->ctx;
  if (!m->nb) return gnx_fail(ctx, GNX_ESTATE, "nb base: model holds no prepared tables");
  NbLaunch L{};
  L.X = dX; L.N = N; L.ldx = ldx; L.C = m->info.C; L.ctx = m->info.ctx; L.M = m->info.M;
  L.W = (int32_t)m->info.W; L.A = m->info.A;
  L.win = m->nb->win; L.tab = m->nb->tab; L.bias = m->nb->bias;
  L.b32 = d_b32; L.b64 = d_b64;
  for (int w0 = 0; w0 < L.W; w0 += 32768) {
    L.w_first = w0;
    const dim3 grid((unsigned)((N + NB_ROWS - 1) / NB_ROWS), (unsigned)std::min(32768, L.W - w0));
    hipLaunchKernelGGL(k_nb_table, grid, dim3(NB_WAVES * 64), 0, ctx->stream, L);
  }
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

extern "C" {

int gnx_model_load_nb(gnx_ctx* ctx, const gnx_model_desc* d, const gnx_nb_window* nb, gnx_model** out) {
  if (!ctx || !out) return GNX_EINVAL;
  *out = nullptr;
  if (!d) return gnx_fail(ctx, GNX_EINVAL, "model description is NULL");
  if (d->base_kind != GNX_BASE_NB) return gnx_fail(ctx, GNX_EINVAL, "gnx_model_load_nb: desc->base_kind must be GNX_BASE_NB");
  if (!nb) return gnx_fail(ctx, GNX_EINVAL, "gnx_model_load_nb: nb array is NULL");
  // geometry checks, smoother and calibrator are gnx_model_load's; the base is added to the model it returns
  gnx_model_desc rest = *d;
  rest.base_kind = GNX_BASE_NONE;
  gnx_model* m = nullptr;
  int rc = gnx_model_load(ctx, &rest, &m);
  if (rc != GNX_OK) return rc;
  m->info.base_kind = GNX_BASE_NB;
  {
    GNX_BIND_DEVICE(ctx);
    rc = nb_build(m, nb);
  }
  if (rc != GNX_OK) {
    const std::string msg = ctx->err;  // (gnx_model_free may not keep it)
    gnx_model_free(m);
    ctx->err = msg;
    return rc;
  }
  *out = m;
  return GNX_OK;
}

int gnx_train_nb_counts_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx,
                            int32_t A, int32_t* d_n1, int32_t* d_n2, int32_t* d_cc) {
  if (!ctx) return GNX_EINVAL;
  int rc = nb_counts_check(ctx, dX, dy, N, ldx, C, M, cx, A, d_n1, d_n2, d_cc);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  HIPCHK(ctx, nb_counts_run(dX, N, ldx, dy, C, M, cx, A, d_n1, d_n2, d_cc, ctx->stream));
  return GNX_OK;
}

int gnx_train_nb_counts(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t cx, int32_t A,
                        int32_t* n1, int32_t* n2, int32_t* cc) {
  if (!ctx) return GNX_EINVAL;
  int rc = nb_counts_check(ctx, X, y, N, ldx, C, M, cx, A, n1, n2, cc);
  if (rc != GNX_OK) return rc;
  const int64_t W = C / M, ldw = M + 2 * cx + (C - M * W);
  for (int64_t i = 0; i < N * W; ++i)
    if (y[i] < 0 || y[i] >= A) return gnx_fail(ctx, GNX_EINVAL, "train_nb_counts: label outside [0, A)");
  for (int64_t n = 0; n < N; ++n)
    for (int64_t j = 0; j < C; ++j)
      if ((uint8_t)X[n * ldx + j] > 2) return gnx_fail(ctx, GNX_EINVAL, "train_nb_counts: X holds a code outside {0, 1, 2}");
  GNX_BIND_DEVICE(ctx);
  const size_t tb = (size_t)W * A * ldw * 4, cb = (size_t)W * A * 4;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_x, (size_t)N * ldx + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, (size_t)N * W * 4)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, 2 * tb + cb)) != GNX_OK) return rc;
  int32_t* d1 = (int32_t*)ctx->ws_misc.p;
  int32_t* d2 = d1 + (size_t)W * A * ldw;
  int32_t* dc = d2 + (size_t)W * A * ldw;
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_x.p, X, (size_t)(N - 1) * ldx + C, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, y, (size_t)N * W * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, nb_counts_run((const int8_t*)ctx->ws_x.p, N, ldx, (const int32_t*)ctx->ws_lab.p, C, M, cx, A, d1, d2, dc, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(n1, d1, tb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(n2, d2, tb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(cc, dc, cb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return GNX_OK;
}

}  // extern "C"
