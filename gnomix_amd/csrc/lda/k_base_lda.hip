// k_base_lda.hip — the LDA base (LDABase) on gfx950: per-window linear decision on the float64 matrix cores with the softmax (or, for
// two classes, the sigmoid) in registers, and the model load behind gnx_model_load_lda.
//
// Replaces LDABase.predict_proba (reference src/Base/models.py through src/Base/base.py:146-180): per window
//   sklearn LinearDiscriminantAnalysis().predict_proba(Xw).
//
// Semantics, complete:
//  * For query haplotype n and window w, with R = A decision rows (R = 1 when A == 2: scikit-learn keeps coef_[1] - coef_[0] only)
//      d[n, r] = sum_p coef[w, r, p] * x[n, col(w, p)] + intercept[w, r]       p = 0 .. width_w - 1
//      A > 2:   B[n, w, :] = softmax_r(d)
//      A == 2:  p = 1 / (1 + exp(-d[n, 0]));  B[n, w, :] = [1 - p, p]
//    col(w, p) is the window's slice of the reflect-padded query (gnx_window.h).  The codes are numbers: 2 = missing is the number 2;
//    a query byte is taken as the signed number it is (k_base_logistic's rule).
//  * coef and intercept are used as the float64 they are: LDA coefficients have no bound that an int8-limb scheme could rely on.
//  * Softmax: m = max_r d; e_r = exp(max(d_r - m, -746)) (gnx_exp.h; float64 exp is 0 from there down); B_r = e_r * (1 / sum e), one
//    reciprocal per row (gnx_rcp_nr).  The largest class has e = 1 exactly, so the sum is in [1, 16].
//    Sigmoid: gnx_sigmoid, the logistic kernels' shared definition.
//  * The float32 output is the float32 rounding of the float64 output.  A <= 16 (one column tile); A > 16 is GNX_EUNSUPPORTED.
//  * Refused at load (GNX_EINVAL): a non-finite coefficient or intercept (the message names the window), a width that is not the
//    window's, n_rows that is not A (or 1 for A == 2), a NULL pointer.
//
// Arithmetic: k_base_logistic's.  v_mfma_f64_16x16x4_f64 takes 16 query rows x 4 positions as the A operand (lane l: row l & 15,
// position l >> 4, the byte converted to float64, exact) and 4 positions x 16 decision columns as the B operand; the products are
// exact (|x| < 2^7) and the accumulator is float64.  Model load lays the coefficients out as (position, 16) doubles, columns >= R and
// positions up to the next multiple of 16 zero, which IS the B-operand stream: one coalesced 512-byte load per four positions.
// Layout (k_nb_table's): a block = one window x LD_ROWS query rows, 4 waves; a wave keeps LD_MT 16-row tiles' accumulators in
// registers and reuses every loaded B operand across them; a lane reads its row's window bytes 16 at a time when the window lies
// inside the unpadded row and gathers byte by byte through the reflected index map otherwise (edge windows, the tail of a width that
// is no multiple of 16; bytes past the width read as 0 against zero coefficients).  The epilogue stays in the accumulator layout
// (column = lane & 15, row = (lane >> 4) + 4 reg): the row maximum and the row sum are butterflies over the 16 lanes of a row.
// No LDS, no scratch, no runtime-indexed register array, plain vector stores.
#include "../gnx_internal.h"
#include "../gnx_exp.h"
#include "../gnx_window.h"

#include <cmath>

struct LdaWinDev {
  int64_t tab_off;  // positions: this window's coefficient rows start at tab[tab_off * 16]
  int32_t width;    // SNPs
  int32_t reserved;
};

struct LdaModel {
  const LdaWinDev* win = nullptr;
  const double* tab = nullptr;   // [sum of widths rounded up to 16][16 columns]
  const double* icpt = nullptr;  // [W][16], 0 in columns >= R
};

struct LdaLaunch {
  const int8_t* X;
  int64_t N, ldx, C, ctx, M;
  int32_t W, A, w_first;
  const LdaWinDev* win;
  const double* tab;
  const double* icpt;
  float* b32;
  double* b64;
};

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(1))) xbytes16 { uint32_t v[4]; };

constexpr int LD_MT = 4;                        // 16-row tiles per wave
constexpr int LD_WAVES = 4;
constexpr int LD_ROWS = LD_WAVES * LD_MT * 16;  // query rows per block
constexpr int LD_PC = 16;                       // positions per X chunk (one 16-byte load per lane)

__device__ __forceinline__ xbytes16 load_x16(const int8_t* p) {  // unaligned global_load_dwordx4
  xbytes16 r;
  __builtin_memcpy(&r, p, 16);
  return r;
}

// positions p0 .. p0 + 15 of the window through the index map; those from the width on read as 0
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

// one chunk of 16 positions = four MFMA steps; tp = the chunk's first coefficient row, this lane's element (position kq, column i16)
__device__ __forceinline__ void lda_chunk(d4 (&acc)[LD_MT], const xbytes16 (&x)[LD_MT], const double* tp, uint32_t kq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double b = tp[(size_t)t * 64];
#pragma unroll
    for (int mt = 0; mt < LD_MT; ++mt) {
      const double a = (double)(int32_t)(int8_t)(x[mt].v[t] >> (8 * kq));  // byte 4 t + kq, sign-extended
      acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[mt], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(LD_WAVES * 64) void k_lda_softmax(LdaLaunch L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15;
  const uint32_t kq = (uint32_t)lane >> 4;
  const int w = L.w_first + blockIdx.y;
  const int64_t n0 = ((int64_t)blockIdx.x * LD_WAVES + wave) * (LD_MT * 16);
  if (n0 >= L.N) return;  // (no block-wide barrier below)
  const LdaWinDev wd = L.win[w];
  const int width = wd.width;
  const int64_t s = (int64_t)w * L.M;  // the window's first position in the reflect-padded row
  const bool contiguous = s >= L.ctx && s + width <= L.ctx + L.C;

  const int8_t* xrow[LD_MT];
#pragma unroll
  for (int mt = 0; mt < LD_MT; ++mt) {
    const int64_t n = n0 + mt * 16 + i16;  // rows past the batch repeat the last one (never written out)
    xrow[mt] = L.X + (n < L.N ? n : L.N - 1) * L.ldx;
  }

  d4 acc[LD_MT];
#pragma unroll
  for (int mt = 0; mt < LD_MT; ++mt) acc[mt] = d4{0.0, 0.0, 0.0, 0.0};

  const double* tp = L.tab + (size_t)wd.tab_off * 16 + lane;
  const int n_full = contiguous ? width / LD_PC : 0;  // chunks served by 16-byte loads: every byte lies inside the row
  int p0 = 0;
  if (n_full > 0) {
    const int64_t c0 = s - L.ctx;
    xbytes16 xn[LD_MT];
#pragma unroll
    for (int mt = 0; mt < LD_MT; ++mt) xn[mt] = load_x16(xrow[mt] + c0);
    for (int c = 0; c < n_full; ++c, p0 += LD_PC) {
      xbytes16 x[LD_MT];
#pragma unroll
      for (int mt = 0; mt < LD_MT; ++mt) x[mt] = xn[mt];
      if (c + 1 < n_full) {
#pragma unroll
        for (int mt = 0; mt < LD_MT; ++mt) xn[mt] = load_x16(xrow[mt] + c0 + p0 + LD_PC);
      }
      lda_chunk(acc, x, tp + (size_t)p0 * 16, kq);
    }
  }
  for (; p0 < width; p0 += LD_PC) {  // reflected windows, and the tail of a contiguous one
    xbytes16 x[LD_MT];
#pragma unroll
    for (int mt = 0; mt < LD_MT; ++mt) x[mt] = gather_x16(xrow[mt], s, p0, width, L.C, L.ctx);
    lda_chunk(acc, x, tp + (size_t)p0 * 16, kq);
  }

  // ---- epilogue in the accumulator layout: column = lane & 15, row = (lane >> 4) + 4 * reg ----
  const double icpt = L.icpt[(size_t)w * 16 + i16];
  const int A = L.A;
  if (A == 2) {  // one decision column: [1 - p, p]
#pragma unroll
    for (int mt = 0; mt < LD_MT; ++mt) {
      double p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = acc[mt][r] + icpt;
      gnx_sigmoidN<4>(p);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = n0 + mt * 16 + (int)kq + 4 * r;
        if (n < L.N && i16 == 0) {
          const size_t o = ((size_t)n * L.W + w) * 2;
          const double q = 1.0 - p[r];
          if (L.b64) { L.b64[o] = q; L.b64[o + 1] = p[r]; }
          if (L.b32) { L.b32[o] = (float)q; L.b32[o + 1] = (float)p[r]; }
        }
      }
    }
    return;
  }
  const bool here = i16 < A;
#pragma unroll
  for (int mt = 0; mt < LD_MT; ++mt) {
    double m[4], e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double d = acc[mt][r] + icpt;
      m[r] = here ? d : -INFINITY;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m[r] = __builtin_fmax(m[r], __shfl_xor(m[r], o, 64));
      e[r] = here ? __builtin_fmax(d - m[r], -746.0) : 0.0;
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
      if (n < L.N && here) {
        const size_t o = ((size_t)n * L.W + w) * A + i16;
        if (L.b64) L.b64[o] = v;
        if (L.b32) L.b32[o] = (float)v;
      }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// model preparation: coefficients in B-operand order, intercepts
// ------------------------------------------------------------------------------------------------
static int lda_build(gnx_model* m, const gnx_lda_window* lda) {
  gnx_ctx* ctx = m->ctx;
  const int A = m->info.A;
  const int R = A == 2 ? 1 : A;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  if (A > 16) return gnx_fail(ctx, GNX_EUNSUPPORTED, "lda base: more than 16 classes (the decision columns are one 16-wide MFMA tile)");
  std::vector<LdaWinDev> wins((size_t)W);
  int64_t rows = 0;
  for (int64_t i = 0; i < W; ++i) {
    const std::string wn = "lda base: window " + std::to_string(i) + ": ";
    const int64_t width = gnx_window_width(i, W, C, M, m->info.ctx);
    if (lda[i].width != width) return gnx_fail(ctx, GNX_EINVAL, wn + "lda[i].width != window width (M+2ctx, +rem for the last)");
    if (lda[i].n_rows != R) return gnx_fail(ctx, GNX_EINVAL, wn + "lda[i].n_rows must be A (1 when A == 2)");
    if (!lda[i].coef || !lda[i].intercept) return gnx_fail(ctx, GNX_EINVAL, wn + "coef / intercept is NULL");
    for (int r = 0; r < R; ++r)
      if (!std::isfinite(lda[i].intercept[r])) return gnx_fail(ctx, GNX_EINVAL, wn + "intercept of row " + std::to_string(r) + " is not finite");
    for (int64_t k = 0; k < (int64_t)R * width; ++k)
      if (!std::isfinite(lda[i].coef[k]))
        return gnx_fail(ctx, GNX_EINVAL, wn + "coefficient of row " + std::to_string(k / width) + ", position " + std::to_string(k % width) + " is not finite");
    wins[(size_t)i] = LdaWinDev{rows, (int32_t)width, 0};
    rows += (width + 15) / 16 * 16;
  }
  std::vector<double> tab((size_t)rows * 16, 0.0), icpt((size_t)W * 16, 0.0);
  for (int64_t i = 0; i < W; ++i) {
    const LdaWinDev& wd = wins[(size_t)i];
    for (int r = 0; r < R; ++r) {
      icpt[(size_t)i * 16 + r] = lda[i].intercept[r];
      for (int64_t p = 0; p < wd.width; ++p) tab[(size_t)(wd.tab_off + p) * 16 + r] = lda[i].coef[(size_t)r * wd.width + p];
    }
  }
  auto md = std::make_shared<LdaModel>();
  int rc;
  if ((rc = gnx_dev_upload(m, wins, &md->win)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, tab, &md->tab)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, icpt, &md->icpt)) != GNX_OK) return rc;
  m->lda = md;
  return GNX_OK;
}

int gnx_base_predict_lda(gnx_model* m, const int8_t* dX, int64_t N, int64_t ldx, float* d_b32, double* d_b64) {
  gnx_ctx* ctx = m->ctx;
  if (!m->lda) return gnx_fail(ctx, GNX_ESTATE, "lda base: model holds no prepared coefficients");
  LdaLaunch L{};
  L.X = dX; L.N = N; L.ldx = ldx; L.C = m->info.C; L.ctx = m->info.ctx; L.M = m->info.M;
  L.W = (int32_t)m->info.W; L.A = m->info.A;
  L.win = m->lda->win; L.tab = m->lda->tab; L.icpt = m->lda->icpt;
  L.b32 = d_b32; L.b64 = d_b64;
  for (int w0 = 0; w0 < L.W; w0 += 32768) {
    L.w_first = w0;
    const dim3 grid((unsigned)((N + LD_ROWS - 1) / LD_ROWS), (unsigned)std::min(32768, L.W - w0));
    hipLaunchKernelGGL(k_lda_softmax, grid, dim3(LD_WAVES * 64), 0, ctx->stream, L);
  }
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

extern "C" {

int gnx_model_load_lda(gnx_ctx* ctx, const gnx_model_desc* d, const gnx_lda_window* lda, gnx_model** out) {
  if (!ctx || !out) return GNX_EINVAL;
  *out = nullptr;
  if (!d) return gnx_fail(ctx, GNX_EINVAL, "model description is NULL");
  if (d->base_kind != GNX_BASE_LDA) return gnx_fail(ctx, GNX_EINVAL, "gnx_model_load_lda: desc->base_kind must be GNX_BASE_LDA");
  if (!lda) return gnx_fail(ctx, GNX_EINVAL, "gnx_model_load_lda: lda array is NULL");
  // geometry checks, smoother and calibrator are gnx_model_load's; the base is added to the model it returns
  gnx_model_desc rest = *d;
  rest.base_kind = GNX_BASE_NONE;
  gnx_model* m = nullptr;
  int rc = gnx_model_load(ctx, &rest, &m);
  if (rc != GNX_OK) return rc;
  m->info.base_kind = GNX_BASE_LDA;
  {
    GNX_BIND_DEVICE(ctx);
    rc = lda_build(m, lda);
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

}  // extern "C"
