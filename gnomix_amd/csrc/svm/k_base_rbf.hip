// k_base_rbf.hip — the RBF SVC base (SVMBase) on gfx950: squared distances on the int8 matrix cores.
//
// Replaces SVMBase.predict_proba (reference src/Base/models.py:148-159 through src/Base/base.py:146-180): per window
//   sklearn SVC(C=100., gamma=0.001, probability=True).predict_proba(Xw)  -> libsvm predict_values (k_function = RBF) /
//   sigmoid_predict / multiclass_probability (sklearn/svm/src/libsvm/svm.cpp, third-party).
//
// The RBF argument is an integer for SNP codes:  |x - y|^2 = |x|^2 + |y|^2 - 2 x.y,  and x.y over int8 codes is what
// v_mfma_i32_16x16x64_i8 computes, exactly.  K = exp(-gamma d2) is then a lookup in a per-(gamma, width) table
// T[k] = exp(-gamma k) that the HOST fills with the C library's exp at model load (gnx_rbf_table): the kernel values equal
// libsvm's on the same host bit for bit, and no float64 exp runs per (query, support vector).
// Design (pass 2a; pass 2b is k_base_covrsk.hip's k_svc_couple*, fed the same r_ij layout):
//  * one block = QB query haplotypes of one window (QB = 64, 32 or 16: the largest whose LDS working set fits), 4 waves;
//  * the queries' window bytes are gathered once into LDS over the reflect-padded coordinate (base.py:41-44; the last window is
//    M_ + rem wide), zero beyond the width; the support rows sit in HBM as zero-padded int8 rows of kp = width rounded up to 64
//    bytes, so 16 aligned bytes of a row ARE the B operand (column = lane & 15, k-block = lane >> 4) and 16 LDS bytes the A operand;
//  * per tile of 64 support vectors each wave accumulates its 16 x 16 int32 tiles over kp / 64 MFMAs, turns them into
//    d2 = |x|^2 + |sv|^2 - 2 acc (integer side sums) and parks them in LDS as [query][65];
//  * thread (query q, pair group g) then walks the tile's support vectors IN ORDER: K = T[d2], and every class pair of its group
//    that involves the vector's class gets  dec += coef * K  in float64, multiply and add rounded separately (-ffp-contract=off)
//    — libsvm's order (class-major, support-vector order inside a class), as k_covrsk_dec;
//  * Platt sigmoids -> r_ij.
// The table stays in global memory (L2 / L1): at width 2 500 it is 180 KB, more than the LDS holds beside the query tile, and a
// window's distances cluster in a narrow band of it (a few cache lines serve a wave's gather).
// Query codes: 0, 1, 2 (2 = missing is the number 2), and 3 (the largest a 2-bit packed row can hold) as the number 3; the table
// covers 9 * width.  Any other int8 value is outside the contract: the distance is clamped to the table's end, never out of bounds.
// The Gram pass of the trainer (k_rbf_stage / k_rbf_gram, used by k_train_svc.hip) is the same arithmetic on N x N rows.
#include "gnx_svc_rbf.h"
#include "../gnx_window.h"

#include <cmath>
#include <cstring>
#include <map>

struct RbfWinDev {
  int32_t width, kp, n_sv, tmax;  // SNPs; row pitch in bytes (width rounded up to 64); support vectors; last table index
  int64_t sv_off;                 // bytes: this window's support rows [n_sv rounded up to 64][kp], zero-padded
  int64_t yy_off;                 // int32 units: |sv|^2 per (padded) support row
  int64_t coef_off;               // doubles: dual (A-1, n_sv) | intercept P | probA P | probB P
  int64_t tab_off;                // doubles: T[0 .. tmax]
  int32_t cls_start[36];          // support-vector index range per class (prefix sums of n_support)
};

struct SvcRbfModel {
  const RbfWinDev* win = nullptr;
  const int8_t* sv = nullptr;
  const int32_t* yy = nullptr;
  const double* coef = nullptr;
  const double* tab = nullptr;
  int QB = 0;
  size_t lds = 0;
};

struct RbfLaunch {
  const int8_t* X;
  int64_t ldx, C, ctx, M;
  int32_t W, A, w_first;
  const RbfWinDev* win;
  const int8_t* sv;
  const int32_t* yy;
  const double* coef;
  const double* tab;
  double* rpair;
  int64_t n_first, n_count;
};

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double sigmoid_predict(double dec, double pa, double pb) {
  const double f = dec * pa + pb;
  if (f >= 0) return exp(-f) / (1.0 + exp(-f));
  return 1.0 / (1.0 + exp(f));
}

__host__ __device__ constexpr size_t r16(size_t b) { return (b + 15) & ~(size_t)15; }

size_t rbf_lds_bytes(int QB, int kp, int P) { return r16((size_t)P * QB * 8) + (size_t)QB * 264 + (size_t)QB * (kp + 16); }

template <int QB>
__global__ __launch_bounds__(256) void k_rbf_dec(RbfLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int MTN = QB / 16;  // 16-query row tiles of the block; a tile step has MTN x 4 MFMA tiles, MTN per wave
  constexpr int G = 256 / QB;   // pair groups: thread (q, g) owns the class pairs p with p % G == g
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int w = L.w_first + blockIdx.y;
  const int A = L.A, P = A * (A - 1) / 2;
  const RbfWinDev* wp = L.win + w;
  const int width = wp->width, kp = wp->kp, n_sv = wp->n_sv, tmax = wp->tmax;
  const int xs = kp + 16;  // LDS row pitch of the query tile

  double* dec = reinterpret_cast<double*>(lds);                                  // [P][QB]
  int32_t* d2s = reinterpret_cast<int32_t*>(lds + r16((size_t)P * QB * 8));      // [QB][65]
  int32_t* xx = d2s + QB * 65;                                                   // [QB]
  int8_t* xq = reinterpret_cast<int8_t*>(xx + QB);                               // [QB][xs]

  const int64_t n0 = L.n_first + (int64_t)blockIdx.x * QB;
  const int64_t n_end = L.n_first + L.n_count;

  // ---- the queries' window bytes over the reflect-padded coordinate; rows past the batch repeat the last one (never written out) ----
  {
    const int64_t s = (int64_t)w * L.M;
    const int total = QB * kp;
    for (int idx = t; idx < total; idx += 256) {
      const int q = idx / kp, k = idx - q * kp;
      const int64_t n = (n0 + q < n_end) ? n0 + q : n_end - 1;
      int8_t v = 0;
      if (k < width) v = L.X[n * L.ldx + gnx_pad_src(s + k, L.C, L.ctx)];
      xq[q * xs + k] = v;
    }
    for (int i = t; i < P * QB; i += 256) dec[i] = 0.0;
    if (t < QB) xx[t] = 0;
  }
  __syncthreads();
  {
    const int q = t % QB, part = t / QB, len = kp / G;  // kp is a multiple of 64, G divides 16
    int sum = 0;
    const int8_t* row = xq + q * xs + part * len;
    for (int k = 0; k < len; ++k) sum += (int)row[k] * (int)row[k];
    atomicAdd(&xx[q], sum);
  }
  __syncthreads();

  const int mt = wv % MTN;
  const int8_t* arow = xq + (mt * 16 + (lane & 15)) * xs + (lane >> 4) * 16;
  const int8_t* svw = L.sv + wp->sv_off;
  const int32_t* yyw = L.yy + wp->yy_off;
  const double* tab = L.tab + wp->tab_off;
  const double* dual = L.coef + wp->coef_off;  // (A-1, n_sv)
  const int32_t* cls_start = wp->cls_start;
  const int q = t % QB, g = t / QB;
  int c = 0;  // class of the support vector being added (vectors are class-major)

  for (int s0 = 0; s0 < n_sv; s0 += 64) {
    v4i acc[MTN];
#pragma unroll
    for (int j = 0; j < MTN; ++j) acc[j] = v4i{0, 0, 0, 0};
    for (int k0 = 0; k0 < kp; k0 += 64) {
      const v4i a = *reinterpret_cast<const v4i*>(arow + k0);
#pragma unroll
      for (int j = 0; j < MTN; ++j) {
        const int nt = (wv + 4 * j) / MTN;
        const v4i b = *reinterpret_cast<const v4i*>(svw + (size_t)(s0 + nt * 16 + (lane & 15)) * kp + k0 + (lane >> 4) * 16);
        acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[j], 0, 0, 0);
      }
    }
    // int32 16x16 C/D layout: column (support vector) = lane & 15, row (query) = 4 * (lane >> 4) + reg
#pragma unroll
    for (int j = 0; j < MTN; ++j) {
      const int nt = (wv + 4 * j) / MTN;
      const int sl = nt * 16 + (lane & 15);
      const int ys = yyw[s0 + sl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ql = mt * 16 + 4 * (lane >> 4) + r;
        int d2 = xx[ql] + ys - 2 * acc[j][r];
        d2 = d2 < 0 ? 0 : (d2 > tmax ? tmax : d2);
        d2s[ql * 65 + sl] = d2;
      }
    }
    __syncthreads();
    // ---- libsvm predict_values order: every pair (i<j) sums its class-i vectors (coef row j-1), then its class-j vectors (row i) ----
    const int send = (n_sv - s0 < 64) ? n_sv - s0 : 64;
    for (int s = 0; s < send; ++s) {
      const int sv = s0 + s;
      while (sv >= cls_start[c + 1]) ++c;
      const double Kd = tab[d2s[q * 65 + s]];
      for (int o = 0; o < A; ++o) {
        if (o == c) continue;
        const int row = (o > c) ? o - 1 : o;
        const int p = (o > c) ? pair_index(c, o, A) : pair_index(o, c, A);
        if (p % G == g) dec[p * QB + q] += dual[(size_t)row * n_sv + sv] * Kd;
      }
    }
    __syncthreads();
  }

  // ---- Platt sigmoids (svm_predict_probability): r_ij, i<j ----
  const double* icpt = dual + (size_t)(A - 1) * n_sv;
  const double* pA = icpt + P;
  const double* pB = pA + P;
  const double min_prob = 1e-7;
  if (n0 + q < n_end) {
    double* out = L.rpair + (((size_t)(n0 + q - L.n_first)) * L.W + w) * P;
    for (int p = g; p < P; p += G) {
      const double d = dec[p * QB + q] + icpt[p];  // sklearn _intercept_ = -rho
      const double v = sigmoid_predict(d, pA[p], pB[p]);
      out[p] = fmin(fmax(v, min_prob), 1 - min_prob);
    }
  }
}

// ---- the trainer's Gram pass ----------------------------------------------------------------------------------------------
// one thread = 4 bytes of one staged row
__global__ __launch_bounds__(256) void k_rbf_stage(const int8_t* X, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t ctx, int w_first,
                                                    int nb, int W, int rem, int64_t Np, int kp, int8_t* xw) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int kq = kp / 4;
  if (idx >= (int64_t)nb * Np * kq) return;
  const int k4 = (int)(idx % kq);
  const int64_t n = (idx / kq) % Np;
  const int wl = (int)(idx / ((int64_t)kq * Np));
  const int w = w_first + wl;
  const int width = (int)(M + 2 * ctx) + (w == W - 1 ? rem : 0);
  uint32_t v = 0;
  if (n < N)
    for (int b = 0; b < 4; ++b) {
      const int k = k4 * 4 + b;
      if (k < width) v |= (uint32_t)(uint8_t)X[n * ldx + gnx_pad_src((int64_t)w * M + k, C, ctx)] << (8 * b);
    }
  reinterpret_cast<uint32_t*>(xw)[idx] = v;
}

__global__ __launch_bounds__(256) void k_rbf_norm(const int8_t* xw, int64_t rows, int kp, int32_t* nrm) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int8_t* x = xw + r * kp;
  int s = 0;
  for (int k = 0; k < kp; ++k) s += (int)x[k] * (int)x[k];
  nrm[r] = s;
}

// 64 x 64 tile of (i, j) of window blockIdx.z: wave v = rows 16 v .. 16 v + 15, four 16-column tiles; both operands straight from
// the staged rows (16 aligned bytes = one lane's operand)
__global__ __launch_bounds__(256) void k_rbf_gram(const int8_t* xw, const int32_t* nrm, int64_t N, int64_t Np, int kp, const double* tab,
                                                   int32_t tmax, float* gram, int32_t* d2o) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wl = blockIdx.z;
  const int8_t* xb = xw + (size_t)wl * Np * kp;
  const int32_t* nb = nrm + (size_t)wl * Np;
  const int64_t i0 = (int64_t)blockIdx.x * 64 + wv * 16, j0 = (int64_t)blockIdx.y * 64;
  const int8_t* ar = xb + (size_t)(i0 + (lane & 15)) * kp + (lane >> 4) * 16;
  v4i acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = v4i{0, 0, 0, 0};
  for (int k0 = 0; k0 < kp; k0 += 64) {
    const v4i a = *reinterpret_cast<const v4i*>(ar + k0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const v4i b = *reinterpret_cast<const v4i*>(xb + (size_t)(j0 + j * 16 + (lane & 15)) * kp + k0 + (lane >> 4) * 16);
      acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[j], 0, 0, 0);
    }
  }
  float* G = gram + (size_t)wl * N * N;
  int32_t* D = d2o + (size_t)wl * N * N;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t cj = j0 + j * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t ri = i0 + 4 * (lane >> 4) + r;
      if (ri < N && cj < N) {
        int d2 = nb[ri] + nb[cj] - 2 * acc[j][r];
        d2 = d2 < 0 ? 0 : (d2 > tmax ? tmax : d2);
        D[ri * N + cj] = d2;
        G[ri * N + cj] = (float)tab[d2];  // libsvm's Qfloat of the double kernel value
      }
    }
  }
}

template <int QB>
hipError_t launch_dec(const RbfLaunch& L, size_t lds, hipStream_t s) {
  GNX_LDS_OPTIN(lds, k_rbf_dec<QB>);
  for (int w0 = 0; w0 < L.W; w0 += 32768) {
    RbfLaunch Lw = L;
    Lw.w_first = w0;
    const dim3 grid((unsigned)((L.n_count + QB - 1) / QB), (unsigned)std::min(32768, L.W - w0));
    hipLaunchKernelGGL(k_rbf_dec<QB>, grid, dim3(256), lds, s, Lw);
  }
  return hipGetLastError();
}

}  // namespace

void gnx_rbf_table(double gamma, int64_t n, std::vector<double>& out) {
  out.resize((size_t)n);
  for (int64_t k = 0; k < n; ++k) out[(size_t)k] = std::exp(-gamma * (double)k);
}

hipError_t gnx_launch_rbf_stage(const int8_t* X, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t ctx, int w_first, int nb, int W,
                                int rem, int64_t Np, int kp, int8_t* xw, int32_t* nrm, hipStream_t s) {
  const int64_t words = (int64_t)nb * Np * (kp / 4), rows = (int64_t)nb * Np;
  hipLaunchKernelGGL(k_rbf_stage, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, X, N, ldx, C, M, ctx, w_first, nb, W, rem, Np, kp, xw);
  hipLaunchKernelGGL(k_rbf_norm, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, xw, rows, kp, nrm);
  return hipGetLastError();
}

hipError_t gnx_launch_rbf_gram(const int8_t* xw, const int32_t* nrm, int64_t N, int64_t Np, int kp, int nb, const double* tab,
                               int32_t tmax, float* gram, int32_t* d2, hipStream_t s) {
  const unsigned tiles = (unsigned)(Np / 64);
  hipLaunchKernelGGL(k_rbf_gram, dim3(tiles, tiles, (unsigned)nb), dim3(256), 0, s, xw, nrm, N, Np, kp, tab, tmax, gram, d2);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// model preparation: support rows as zero-padded int8 rows, their norms, the exp table(s)
// ------------------------------------------------------------------------------------------------
int gnx_build_svc_rbf(gnx_model* m, const gnx_model_desc* d) {
  gnx_ctx* ctx = m->ctx;
  const int A = d->A, P = A * (A - 1) / 2;
  const int64_t C = d->C, M = d->M, W = C / M, rem = C - M * W, M_ = M + 2 * d->ctx;
  if (!d->svc) return gnx_fail(ctx, GNX_EINVAL, "rbf base: svc array is NULL");
  // the shared coupling pass (k_svc_couple: P + A*A + 2A doubles x 64 lanes in LDS) is validated up to the CovRSK base's limit
  if (A > GNX_RBF_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, "rbf base: more than GNX_RBF_MAX_A (13) ancestries");
  std::vector<RbfWinDev> wins((size_t)W);
  std::vector<int8_t> sv;
  std::vector<int32_t> yy;
  std::vector<double> coef, tab, tmp;
  std::map<std::pair<uint64_t, int64_t>, int64_t> tabs;  // (gamma bits, width) -> offset
  int max_kp = 0;
  for (int64_t i = 0; i < W; ++i) {
    const gnx_svc_window& sw = d->svc[i];
    const std::string wn = "rbf base: window " + std::to_string(i) + ": ";
    const int64_t width = (i == W - 1) ? M_ + rem : M_;
    if (sw.kernel_kind != GNX_SVC_KERNEL_RBF) return gnx_fail(ctx, GNX_EINVAL, wn + "kernel_kind differs from window 0's (GNX_SVC_KERNEL_RBF)");
    if (sw.width != width) return gnx_fail(ctx, GNX_EINVAL, wn + "svc[i].width != window width (M+2ctx, +rem for the last)");
    if (width > GNX_RBF_MAX_WIDTH) return gnx_fail(ctx, GNX_EINVAL, wn + "wider than GNX_RBF_MAX_WIDTH SNPs");
    if (!(sw.gamma > 0.0) || !std::isfinite(sw.gamma)) return gnx_fail(ctx, GNX_EINVAL, wn + "gamma must be finite and > 0");
    if (!sw.xfit || !sw.support || !sw.dual_coef || !sw.intercept || !sw.prob_a || !sw.prob_b || !sw.n_support || sw.n_sv <= 0)
      return gnx_fail(ctx, GNX_EINVAL, wn + "incomplete svc window");
    RbfWinDev& wd = wins[(size_t)i];
    std::memset(&wd, 0, sizeof(wd));
    wd.width = (int32_t)width;
    wd.kp = (int32_t)((width + 63) / 64 * 64);
    wd.n_sv = sw.n_sv;
    max_kp = std::max(max_kp, wd.kp);
    int acc = 0;
    for (int c = 0; c < A; ++c) {
      if (sw.n_support[c] < 0) return gnx_fail(ctx, GNX_EINVAL, wn + "negative n_support");
      wd.cls_start[c] = acc;
      acc += sw.n_support[c];
    }
    wd.cls_start[A] = acc;
    if (acc != sw.n_sv) return gnx_fail(ctx, GNX_EINVAL, wn + "sum(n_support) != n_sv");
    const int64_t tlen = gnx_rbf_table_len(width);
    wd.tmax = (int32_t)(tlen - 1);
    uint64_t gbits;
    std::memcpy(&gbits, &sw.gamma, 8);
    auto it = tabs.find({gbits, width});
    if (it == tabs.end()) {
      gnx_rbf_table(sw.gamma, tlen, tmp);
      it = tabs.emplace(std::make_pair(gbits, width), (int64_t)tab.size()).first;
      tab.insert(tab.end(), tmp.begin(), tmp.end());
    }
    wd.tab_off = it->second;
    const int64_t n_svp = ((int64_t)sw.n_sv + 63) / 64 * 64;
    wd.sv_off = (int64_t)sv.size();
    wd.yy_off = (int64_t)yy.size();
    sv.resize(sv.size() + (size_t)n_svp * wd.kp, 0);
    yy.resize(yy.size() + (size_t)n_svp, 0);
    for (int k = 0; k < sw.n_sv; ++k) {
      const int32_t r = sw.support[k];
      if (r < 0 || r >= sw.n_fit) return gnx_fail(ctx, GNX_EINVAL, wn + "support index out of range");
      const int8_t* row = sw.xfit + (size_t)r * width;
      int8_t* dst = sv.data() + wd.sv_off + (size_t)k * wd.kp;
      int32_t s2 = 0;
      for (int64_t t = 0; t < width; ++t) {
        const int8_t v = row[t];
        if (v < 0 || v > 2) return gnx_fail(ctx, GNX_EINVAL, wn + "support row " + std::to_string(k) + " holds " + std::to_string((int)v) +
                                                            " at SNP " + std::to_string(t) + " (codes must be 0..2)");
        dst[t] = v;
        s2 += (int32_t)v * v;
      }
      yy[(size_t)wd.yy_off + k] = s2;
    }
    wd.coef_off = (int64_t)coef.size();
    coef.insert(coef.end(), sw.dual_coef, sw.dual_coef + (size_t)(A - 1) * sw.n_sv);
    coef.insert(coef.end(), sw.intercept, sw.intercept + P);
    coef.insert(coef.end(), sw.prob_a, sw.prob_a + P);
    coef.insert(coef.end(), sw.prob_b, sw.prob_b + P);
  }
  auto rbf = std::make_shared<SvcRbfModel>();
  for (int QB : {64, 32, 16})
    if (rbf_lds_bytes(QB, max_kp, P) <= (size_t)160 * 1024) { rbf->QB = QB; break; }
  if (!rbf->QB) return gnx_fail(ctx, GNX_EUNSUPPORTED, "rbf base: window too wide for the LDS working set");
  rbf->lds = rbf_lds_bytes(rbf->QB, max_kp, P);
  int rc;
  if ((rc = gnx_dev_upload(m, wins, &rbf->win)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, sv, &rbf->sv, 64)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, yy, &rbf->yy)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, coef, &rbf->coef)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, tab, &rbf->tab)) != GNX_OK) return rc;
  m->rbf = rbf;
  return GNX_OK;
}

int gnx_base_predict_rbf(gnx_model* m, const int8_t* dX, int64_t N, int64_t ldx, float* d_b32, double* d_b64) {
  gnx_ctx* ctx = m->ctx;
  const SvcRbfModel& R = *m->rbf;
  const int A = m->info.A, P = A * (A - 1) / 2;
  const size_t per_hap = (size_t)m->info.W * P * sizeof(double);
  int64_t haps = std::max<int64_t>(64, (((int64_t)256 << 20) / (int64_t)per_hap) / 64 * 64);
  haps = std::min<int64_t>(haps, (N + 63) / 64 * 64);
  int rc = gnx_ws_reserve(ctx, ctx->ws_rpair, (size_t)haps * per_hap);
  if (rc != GNX_OK) return rc;
  RbfLaunch L{};
  L.X = dX; L.ldx = ldx; L.C = m->info.C; L.ctx = m->info.ctx; L.M = m->info.M;
  L.W = (int32_t)m->info.W; L.A = A;
  L.win = R.win; L.sv = R.sv; L.yy = R.yy; L.coef = R.coef; L.tab = R.tab;
  L.rpair = (double*)ctx->ws_rpair.p;
  CovRSKLaunch Lc{};  // pass 2b reads W, A, rpair, the chunk and the outputs
  Lc.N = N; Lc.W = L.W; Lc.A = A; Lc.rpair = L.rpair; Lc.b32 = d_b32; Lc.b64 = d_b64;
  for (int64_t n0 = 0; n0 < N; n0 += haps) {
    L.n_first = n0;
    L.n_count = std::min<int64_t>(haps, N - n0);
    switch (R.QB) {
      case 64: HIPCHK(ctx, launch_dec<64>(L, R.lds, ctx->stream)); break;
      case 32: HIPCHK(ctx, launch_dec<32>(L, R.lds, ctx->stream)); break;
      default: HIPCHK(ctx, launch_dec<16>(L, R.lds, ctx->stream)); break;
    }
    Lc.n_first = L.n_first; Lc.n_count = L.n_count;
    HIPCHK(ctx, gnx_launch_svc_couple(Lc, ctx->stream));
  }
  return GNX_OK;
}
