// k_train_lr.hip — training the per-window logistic base on the device.
//
// Reference: Gnomix.train -> Base.train -> per window `LogisticRegression(penalty="l2", C=3., solver="liblinear",
// max_iter=1000).fit(X_w, y_w)` (src/model.py:104-167, src/Base/base.py:104-127, src/Base/models.py:12-21).  X_w is the
// window's slice of the reflect-padded chromosome (base.py:41-44, 111-127), y_w the window's ancestry labels.  liblinear's
// L2R_LR primal problem, one-vs-rest for A >= 3 (one binary problem "class a against the rest" per class; A == 2 is ONE
// problem whose positive class is 1, sklearn keeps a single coefficient row), bias as an extra REGULARISED feature of value 1
// (fit_intercept=True, intercept_scaling=1):
//
//        min_w  f(w) = 1/2 w'w + C sum_i log(1 + exp(-y_i w'x_i)),      x_i = [window SNPs in {0,1,2}, 1]
//
// f is strictly convex, so the fit is DEFINED by its unique minimiser; liblinear approaches it with a trust-region / line
// search Newton method and stops at a relative gradient tolerance (tol = 1e-4).  This file minimises the same f for all
// W x A problems of a chromosome at once, in float64, with a Newton method of the same family (preconditioned CG on
// H = I + C X'DX, Armijo backtracking), run to a tighter tolerance: the result is the optimum the reference's solver
// approximates, and `tests/test_gpu_train.py` checks f(ours) <= f(reference) and coefficient / probability agreement at the
// size of the reference's own stopping error (golden G16 is sklearn's fit through the reference's Base.train).
//
// Data movement per product: the problems of a window share the window's SNPs, so X.v for all classes is one pass over the
// window's bytes (forward: thread = haplotype, weights broadcast from LDS) and X'.r one pass in the other direction
// (backward: thread = SNP, a tile of haplotypes x SNPs staged through LDS).  float64 FMAs on the vector ALU: the products are
// HBM/L2-bound int8 reads against ~7 multiply-adds per byte — the matrix pipe would need the operands quantised per
// iteration and is not worth it for a one-off training pass.
#include <cmath>
#include <cstdio>
#include <vector>

#include "gnx_internal.h"
#include "gnx_window.h"

namespace {

struct Geom {
  int64_t N, ldx, C, M, ctx;
  int32_t W, A, npw;   // npw = problems per window: A (one-vs-rest) or 1 (A == 2)
  int32_t len, len_last, ldw;  // window widths (M + 2ctx, + C mod M for the last), row stride of the weight arrays (= len_last + 1)
};

constexpr int AMAX = 32;
constexpr int FH = 2;    // haplotypes per thread in the forward product
constexpr int FKC = 128;  // SNPs per LDS chunk of the weights

// Z[n, w, p] = sum_k V[(w,p), k] * xp[n, w*M + k] + V[(w,p), ldw-1]          (ldw-1 = the bias element)
// NP = compile-time bound of the per-window problem count (accumulators indexed by a run-time class would live in scratch)
template <int NP>
__global__ __launch_bounds__(128) void k_tr_forward(Geom g, const int8_t* __restrict__ X, const double* __restrict__ V,
                                                    double* __restrict__ Z) {
  __shared__ double vs[FKC * AMAX];
  const int w = blockIdx.y, tid = threadIdx.x;
  const int npw = g.npw;
  const int len = (w == g.W - 1) ? g.len_last : g.len;
  const int64_t start = (int64_t)w * g.M;
  const double* Vw = V + (size_t)w * npw * g.ldw;
  int64_t n[FH];
  const int8_t* row[FH];
#pragma unroll
  for (int h = 0; h < FH; ++h) {
    n[h] = ((int64_t)blockIdx.x * blockDim.x + tid) * FH + h;
    row[h] = X + (n[h] < g.N ? n[h] : g.N - 1) * g.ldx;
  }
  double acc[FH][NP];
#pragma unroll
  for (int h = 0; h < FH; ++h)
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[h][p] = 0.0;
  // no reflect padding inside this window, and the 16-byte loads (which may overrun the window's end by < 16 bytes) stay
  // inside the row
  const bool inner = start >= g.ctx && start + ((len + 15) & ~15) <= g.ctx + g.C;
  for (int k0 = 0; k0 < len; k0 += FKC) {
    const int kc = min(FKC, len - k0);
    __syncthreads();
    for (int e = tid; e < kc * NP; e += blockDim.x) {
      const int p = e / kc, k = e - p * kc;
      vs[k * AMAX + p] = p < npw ? Vw[(size_t)p * g.ldw + k0 + k] : 0.0;
    }
    __syncthreads();
    if (inner) {
      // 16 SNPs per load: a lane streams ITS row (one 128-byte line serves 8 consecutive loads); bytes past the window's end
      // (kc not a multiple of 16) are read but multiplied by nothing
      for (int k = 0; k < kc; k += 16) {
        uint32_t q[FH][4];
#pragma unroll
        for (int h = 0; h < FH; ++h) __builtin_memcpy(q[h], row[h] + (start + k0 + k - g.ctx), 16);
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          if (k + b < kc) {
            double x[FH];
#pragma unroll
            for (int h = 0; h < FH; ++h) x[h] = (double)((q[h][b >> 2] >> (8 * (b & 3))) & 0xffu);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
              const double v = vs[(k + b) * AMAX + p];   // rows of vs past npw hold zeros
#pragma unroll
              for (int h = 0; h < FH; ++h) acc[h][p] = fma(v, x[h], acc[h][p]);
            }
          }
        }
      }
    } else {
      for (int k = 0; k < kc; ++k) {
        double x[FH];
#pragma unroll
        for (int h = 0; h < FH; ++h) x[h] = (double)row[h][gnx_pad_src(start + k0 + k, g.C, g.ctx)];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const double v = vs[k * AMAX + p];
#pragma unroll
          for (int h = 0; h < FH; ++h) acc[h][p] = fma(v, x[h], acc[h][p]);
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < FH; ++h)
    if (n[h] < g.N) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
        if (p < npw) Z[((size_t)n[h] * g.W + w) * npw + p] = acc[h][p] + Vw[(size_t)p * g.ldw + g.ldw - 1];
    }
}

constexpr int BK = 256;  // SNPs per block of the backward product (thread = SNP)
constexpr int BN = 32;   // haplotypes per LDS tile

// G[(w,p), k] = sum_n xp[n, w*M + k]^(1 or 2) * R[n, w, p]  (k < len);   G[(w,p), ldw-1] = sum_n R[n, w, p]
// SQUARE = true gives the diagonal of X'DX (the Jacobi preconditioner) from R = D.
template <bool SQUARE, int NP>
__global__ __launch_bounds__(BK) void k_tr_backward(Geom g, const int8_t* __restrict__ X, const double* __restrict__ R,
                                                    double* __restrict__ G) {
  __shared__ __attribute__((aligned(16))) uint8_t xt[BN][BK];
  __shared__ double rs[BN][AMAX];
  const int w = blockIdx.y, tid = threadIdx.x;
  const int npw = g.npw;
  const int len = (w == g.W - 1) ? g.len_last : g.len;
  const int k0 = blockIdx.x * BK;
  if (k0 >= len + 1) return;  // (the bias rides in the block that owns k == len)
  const int64_t start = (int64_t)w * g.M;
  const int k = k0 + tid;
  // the whole BK-wide tile lies inside the window and inside the row: plain 16-byte loads (columns past the window's end or
  // the bias column make the block take the per-byte path)
  const bool tile_inner = k0 + BK <= len && start + k0 >= g.ctx && start + k0 + BK <= g.ctx + g.C;
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0;
  for (int64_t n0 = 0; n0 < g.N; n0 += BN) {
    __syncthreads();
    if (tile_inner) {  // 16 bytes per load, 16 lanes along a row
      for (int e = tid; e < BN * (BK / 16); e += BK) {
        const int r = e / (BK / 16), c = (e - r * (BK / 16)) * 16;
        const int64_t n = n0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (n < g.N) __builtin_memcpy(&v, X + n * g.ldx + (start + k0 + c - g.ctx), 16);
        *reinterpret_cast<uint4*>(&xt[r][c]) = v;
      }
    } else {
      for (int e = tid; e < BN * BK; e += BK) {
        const int r = e / BK, c = e - r * BK;
        const int64_t n = n0 + r, pp = start + k0 + c;
        uint8_t v = 0;
        if (n < g.N && k0 + c < len) v = (uint8_t)X[n * g.ldx + gnx_pad_src(pp, g.C, g.ctx)];
        else if (n < g.N && k0 + c == len) v = 1;  // the bias feature
        xt[r][c] = v;
      }
    }
    for (int e = tid; e < BN * NP; e += BK) {
      const int r = e / NP, p = e - r * NP;
      const int64_t n = n0 + r;
      rs[r][p] = (n < g.N && p < npw) ? R[((size_t)n * g.W + w) * npw + p] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < BN; ++r) {
      double x = (double)xt[r][tid];
      if (SQUARE) x *= x;
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] = fma(x, rs[r][p], acc[p]);
    }
  }
  if (k <= len) {
    const int kk = (k == len) ? g.ldw - 1 : k;
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < npw) G[((size_t)w * npw + p) * g.ldw + kk] = acc[p];
  }
}

__device__ __forceinline__ double log1pexp(double t) {  // log(1 + exp(t)) without overflow
  return t > 0 ? t + log1p(exp(-t)) : log1p(exp(t));
}

__device__ __forceinline__ double yval(const Geom& g, const int32_t* Y, int64_t n, int w, int p) {
  const int lab = Y[(size_t)n * g.W + w];
  return (g.npw == 1 ? lab == 1 : lab == p) ? 1.0 : -1.0;
}

// per sample and problem, with t = y (z + alpha_p zs):
//   MODE 0: loss[P] += Creg log(1 + exp(-t))                                   (line search / objective)
//   MODE 1: R = Creg (sigma(t) - 1) y ;  D = Creg sigma(t) (1 - sigma(t)) ; loss as MODE 0       (gradient + Hessian weights)
//   MODE 2: R = D * Zs                                                          (Hessian-vector product, inner factor)
template <int MODE>
__global__ __launch_bounds__(256) void k_tr_sample(Geom g, double Creg, const int32_t* __restrict__ Y, const double* __restrict__ Z,
                                                   const double* __restrict__ Zs, const double* __restrict__ alpha,
                                                   double* __restrict__ R, double* __restrict__ D, double* __restrict__ loss) {
  __shared__ double part[256];
  const int w = blockIdx.x, npw = g.npw, tid = threadIdx.x;
  for (int p = 0; p < npw; ++p) {
    const double a = (MODE != 2 && alpha && Zs) ? alpha[w * npw + p] : 0.0;
    double s = 0.0;
    for (int64_t n = (int64_t)blockIdx.y * 256 + tid; n < g.N; n += (int64_t)gridDim.y * 256) {
      const size_t i = ((size_t)n * g.W + w) * npw + p;
      if (MODE == 2) { R[i] = D[i] * Zs[i]; continue; }
      const double y = yval(g, Y, n, w, p);
      const double t = y * (Z[i] + (a != 0.0 ? a * Zs[i] : 0.0));
      s += Creg * log1pexp(-t);
      if (MODE == 1) {
        const double sg = 1.0 / (1.0 + exp(-t));
        R[i] = Creg * (sg - 1.0) * y;
        D[i] = Creg * sg * (1.0 - sg);
      }
    }
    if (MODE != 2) {
      part[tid] = s;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
      }
      if (tid == 0) atomicAdd(&loss[w * npw + p], part[0]);
      __syncthreads();
    }
  }
}

// ---- per-problem vector algebra on (P, ldw) arrays: one block per problem -------------------------------------------------
enum { V_DOT = 0, V_AXPY = 1, V_XPBY = 2, V_COPY = 3, V_DIV = 4, V_ADD = 5, V_PRECOND = 6, V_ZAXPY = 7 };

//   V_DOT     out[p]  = <a, b>
//   V_AXPY    a      += s[p] * b                 (masked: s read per problem, skipped where act[p] == 0)
//   V_XPBY    a       = b + s[p] * a
//   V_COPY    a       = b
//   V_DIV     a       = b / c
//   V_ADD     a       = b + c
//   V_PRECOND a       = (1 - 0.01) + 0.01 * (1 + b)      (liblinear's damped Jacobi preconditioner, b = diag(C X'DX))
//   V_ZAXPY   a       = b + s[p] * c
template <int OP>
__global__ __launch_bounds__(256) void k_tr_vec(int ldw, double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ c,
                                                const double* __restrict__ s, const int32_t* __restrict__ act, double* __restrict__ out,
                                                double sign) {
  __shared__ double part[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (act && !act[p] && OP != V_DOT) return;
  const size_t o = (size_t)p * ldw;
  double acc = 0.0;
  const double sc = s ? sign * s[p] : sign;
  for (int k = tid; k < ldw; k += 256) {
    if (OP == V_DOT) acc = fma(a[o + k], b[o + k], acc);
    else if (OP == V_AXPY) a[o + k] = fma(sc, b[o + k], a[o + k]);
    else if (OP == V_XPBY) a[o + k] = fma(sc, a[o + k], b[o + k]);
    else if (OP == V_COPY) a[o + k] = b[o + k];
    else if (OP == V_DIV) a[o + k] = b[o + k] / c[o + k];
    else if (OP == V_ADD) a[o + k] = b[o + k] + c[o + k];
    else if (OP == V_PRECOND) a[o + k] = 0.99 + 0.01 * (1.0 + b[o + k]);
    else if (OP == V_ZAXPY) a[o + k] = fma(sc, c[o + k], b[o + k]);
  }
  if (OP == V_DOT) {
    part[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) part[tid] += part[tid + h];
      __syncthreads();
    }
    if (tid == 0) out[p] = part[0];
  }
}

}  // namespace

// Newton-CG for all P = W * npw problems in lockstep; per-problem step lengths, masks and stopping.
hipError_t gnx_train_lr_run(const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dY, int64_t C, int64_t M, int64_t ctx, int A,
                            double Creg, double tol, int max_newton, int max_cg, double* h_coef, int64_t ldc, double* h_icpt,
                            gnx_train_info* info, hipStream_t st) {
  Geom g{};
  g.N = N; g.ldx = ldx; g.C = C; g.M = M; g.ctx = ctx;
  g.W = (int32_t)(C / M); g.A = A; g.npw = (A == 2) ? 1 : A;
  g.len = (int32_t)(M + 2 * ctx); g.len_last = g.len + (int32_t)(C - M * g.W); g.ldw = g.len_last + 1;
  const int W = g.W, npw = g.npw, P = W * npw, ldw = g.ldw;
  const size_t PV = (size_t)P * ldw, NS = (size_t)N * W * npw;

  gnx_dev_tmp mem[18];  // the 17 float64 arrays below and act
  int n_mem = 0;
  auto zeros = [&](double*& out, size_t n) -> hipError_t {
    gnx_dev_tmp& m = mem[n_mem++];
    GNX_HIPRET(m.alloc(n * sizeof(double)));
    out = m.as<double>();
    return hipMemset(out, 0, n * sizeof(double));
  };
  double *w, *grad, *s, *r, *d, *Hd, *zv, *pre, *Z, *Zs, *R, *D, *sc1, *sc2, *sc3, *loss, *loss_try;
  for (double** a : {&w, &grad, &s, &r, &d, &Hd, &zv, &pre}) GNX_HIPRET(zeros(*a, PV));
  for (double** a : {&Z, &Zs, &R, &D}) GNX_HIPRET(zeros(*a, NS));
  for (double** a : {&sc1, &sc2, &sc3, &loss, &loss_try}) GNX_HIPRET(zeros(*a, (size_t)P));
  GNX_HIPRET(mem[n_mem].alloc((size_t)P * sizeof(int32_t)));
  int32_t* const act = mem[n_mem].as<int32_t>();

  const dim3 fgrid((unsigned)((N + 128 * FH - 1) / (128 * FH)), (unsigned)W);
  const dim3 bgrid((unsigned)((g.len_last + 1 + BK - 1) / BK), (unsigned)W);
  const dim3 sgrid((unsigned)W, (unsigned)std::min<int64_t>(64, (N + 255) / 256));
#define GNX_TR_NP(CALL)                                   \
  if (npw <= 1) { CALL(1) } else if (npw <= 4) { CALL(4) } else if (npw <= 8) { CALL(8) } else if (npw <= 16) { CALL(16) } else { CALL(32) }
#define GNX_TR_FWD(NP_) hipLaunchKernelGGL(k_tr_forward<NP_>, fgrid, dim3(128), 0, st, g, dX, V, Zout);
#define GNX_TR_BWD(NP_) hipLaunchKernelGGL((k_tr_backward<false, NP_>), bgrid, dim3(BK), 0, st, g, dX, Rin, Gout);
#define GNX_TR_BSQ(NP_) hipLaunchKernelGGL((k_tr_backward<true, NP_>), bgrid, dim3(BK), 0, st, g, dX, Rin, Gout);
  auto forward = [&](const double* V, double* Zout) { GNX_TR_NP(GNX_TR_FWD) };
  auto backward = [&](const double* Rin, double* Gout) { GNX_TR_NP(GNX_TR_BWD) };
  auto backward_sq = [&](const double* Rin, double* Gout) { GNX_TR_NP(GNX_TR_BSQ) };
  auto vdot = [&](const double* a, const double* b, double* out) {
    hipLaunchKernelGGL(k_tr_vec<V_DOT>, dim3(P), dim3(256), 0, st, ldw, const_cast<double*>(a), b, nullptr, nullptr, nullptr, out, 1.0);
  };
  std::vector<double> h1((size_t)P), h2((size_t)P), h3((size_t)P), hf((size_t)P), hfold((size_t)P), gnorm0((size_t)P), step((size_t)P);
  std::vector<int32_t> hact((size_t)P, 1), done((size_t)P, 0);
  auto pull = [&](const double* a, std::vector<double>& h) -> hipError_t {
    GNX_HIPRET(hipMemcpyAsync(h.data(), a, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
  };
  auto push = [&](const std::vector<double>& h, double* a) -> hipError_t {
    return hipMemcpyAsync(a, h.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice, st);
  };
  auto push_act = [&](const std::vector<int32_t>& h) -> hipError_t {
    GNX_HIPRET(hipMemcpyAsync(act, h.data(), (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return hipStreamSynchronize(st);  // the host vector is reused right away
  };
  // f, gradient and Hessian weights at the current w (Z = X w is kept up to date by the caller)
  auto eval_grad = [&]() -> hipError_t {
    GNX_HIPRET(hipMemsetAsync(loss, 0, (size_t)P * sizeof(double), st));
    hipLaunchKernelGGL(k_tr_sample<1>, sgrid, dim3(256), 0, st, g, Creg, dY, Z, nullptr, nullptr, R, D, loss);
    backward(R, grad);
    hipLaunchKernelGGL(k_tr_vec<V_ADD>, dim3(P), dim3(256), 0, st, ldw, grad, grad, w, nullptr, nullptr, nullptr, 1.0);  // + w
    vdot(w, w, sc1);
    vdot(grad, grad, sc2);
    GNX_HIPRET(pull(loss, hf));
    GNX_HIPRET(pull(sc1, h1));
    GNX_HIPRET(pull(sc2, h2));
    for (int p = 0; p < P; ++p) hf[(size_t)p] += 0.5 * h1[(size_t)p];
    return hipGetLastError();
  };

  // w = 0: Z = 0 already
  GNX_HIPRET(eval_grad());
  for (int p = 0; p < P; ++p) gnorm0[(size_t)p] = std::sqrt(h2[(size_t)p]);
  int newton = 0, cg_total = 0;
  for (; newton < max_newton; ++newton) {
    int n_act = 0;
    for (int p = 0; p < P; ++p) {
      const bool conv = std::sqrt(h2[(size_t)p]) <= tol * gnorm0[(size_t)p] || gnorm0[(size_t)p] == 0.0;
      if (conv) done[(size_t)p] = 1;
      hact[(size_t)p] = done[(size_t)p] ? 0 : 1;
      n_act += hact[(size_t)p];
    }
    if (n_act == 0) break;
    GNX_HIPRET(push_act(hact));
    // ---- preconditioned CG on H s = -g, H v = v + X'(D .* X v) ----
    backward_sq(D, pre);
    hipLaunchKernelGGL(k_tr_vec<V_PRECOND>, dim3(P), dim3(256), 0, st, ldw, pre, pre, nullptr, nullptr, nullptr, nullptr, 1.0);
    GNX_HIPRET(hipMemsetAsync(s, 0, PV * sizeof(double), st));
    hipLaunchKernelGGL(k_tr_vec<V_COPY>, dim3(P), dim3(256), 0, st, ldw, r, grad, nullptr, nullptr, nullptr, nullptr, 1.0);
    hipLaunchKernelGGL(k_tr_vec<V_AXPY>, dim3(P), dim3(256), 0, st, ldw, r, grad, nullptr, nullptr, nullptr, nullptr, -2.0);  // r = -g
    hipLaunchKernelGGL(k_tr_vec<V_DIV>, dim3(P), dim3(256), 0, st, ldw, zv, r, pre, nullptr, nullptr, nullptr, 1.0);
    hipLaunchKernelGGL(k_tr_vec<V_COPY>, dim3(P), dim3(256), 0, st, ldw, d, zv, nullptr, nullptr, nullptr, nullptr, 1.0);
    vdot(zv, r, sc1);
    std::vector<double> ztr((size_t)P), ztr0((size_t)P);
    GNX_HIPRET(pull(sc1, ztr));
    ztr0 = ztr;
    std::vector<int32_t> cact = hact;
    for (int it = 0; it < max_cg; ++it) {
      int nc = 0;
      for (int p = 0; p < P; ++p) {
        // inexact Newton: the CG residual is driven 100 x below the gradient (liblinear stops at 0.5; the tighter solve
        // costs CG steps and saves Newton steps, each of which is a full round of passes plus a host round trip)
        if (cact[(size_t)p] && (ztr[(size_t)p] <= 1e-4 * ztr0[(size_t)p] || ztr[(size_t)p] <= 0.0)) cact[(size_t)p] = 0;
        nc += cact[(size_t)p];
      }
      if (nc == 0) break;
      GNX_HIPRET(push_act(cact));
      forward(d, Zs);
      hipLaunchKernelGGL(k_tr_sample<2>, sgrid, dim3(256), 0, st, g, Creg, dY, Z, Zs, nullptr, R, D, nullptr);
      backward(R, Hd);
      hipLaunchKernelGGL(k_tr_vec<V_ADD>, dim3(P), dim3(256), 0, st, ldw, Hd, Hd, d, nullptr, nullptr, nullptr, 1.0);
      vdot(d, Hd, sc2);
      GNX_HIPRET(pull(sc2, h3));
      std::vector<double> al((size_t)P, 0.0);
      for (int p = 0; p < P; ++p)
        if (cact[(size_t)p]) al[(size_t)p] = h3[(size_t)p] > 0 ? ztr[(size_t)p] / h3[(size_t)p] : 0.0;
      GNX_HIPRET(push(al, sc3));
      hipLaunchKernelGGL(k_tr_vec<V_AXPY>, dim3(P), dim3(256), 0, st, ldw, s, d, nullptr, sc3, act, nullptr, 1.0);
      hipLaunchKernelGGL(k_tr_vec<V_AXPY>, dim3(P), dim3(256), 0, st, ldw, r, Hd, nullptr, sc3, act, nullptr, -1.0);
      hipLaunchKernelGGL(k_tr_vec<V_DIV>, dim3(P), dim3(256), 0, st, ldw, zv, r, pre, nullptr, act, nullptr, 1.0);
      vdot(zv, r, sc1);
      std::vector<double> znew((size_t)P);
      GNX_HIPRET(pull(sc1, znew));
      std::vector<double> beta((size_t)P, 0.0);
      for (int p = 0; p < P; ++p)
        if (cact[(size_t)p]) { beta[(size_t)p] = ztr[(size_t)p] > 0 ? znew[(size_t)p] / ztr[(size_t)p] : 0.0; ztr[(size_t)p] = znew[(size_t)p]; }
      GNX_HIPRET(push(beta, sc3));
      hipLaunchKernelGGL(k_tr_vec<V_XPBY>, dim3(P), dim3(256), 0, st, ldw, d, zv, nullptr, sc3, act, nullptr, 1.0);  // d = z + beta d
      ++cg_total;
    }
    // ---- Armijo backtracking along s: f(w + a s) <= f(w) + eta a g's ----
    GNX_HIPRET(push_act(hact));
    forward(s, Zs);
    vdot(grad, s, sc1);
    vdot(s, s, sc2);
    vdot(w, s, sc3);
    std::vector<double> gs((size_t)P), ss((size_t)P), ws((size_t)P), ww((size_t)P);
    GNX_HIPRET(pull(sc1, gs));
    GNX_HIPRET(pull(sc2, ss));
    GNX_HIPRET(pull(sc3, ws));
    vdot(w, w, sc1);
    GNX_HIPRET(pull(sc1, ww));
    hfold = hf;
    std::vector<int32_t> ls = hact;
    for (int p = 0; p < P; ++p) step[(size_t)p] = hact[(size_t)p] ? 1.0 : 0.0;
    for (int bt = 0; bt < 30; ++bt) {
      int nl = 0;
      for (int p = 0; p < P; ++p) nl += ls[(size_t)p];
      if (nl == 0) break;
      GNX_HIPRET(push(step, sc3));
      GNX_HIPRET(hipMemsetAsync(loss_try, 0, (size_t)P * sizeof(double), st));
      hipLaunchKernelGGL(k_tr_sample<0>, sgrid, dim3(256), 0, st, g, Creg, dY, Z, Zs, sc3, nullptr, nullptr, loss_try);
      GNX_HIPRET(pull(loss_try, h3));
      for (int p = 0; p < P; ++p) {
        if (!ls[(size_t)p]) continue;
        const double a = step[(size_t)p];
        const double fnew = h3[(size_t)p] + 0.5 * (ww[(size_t)p] + 2 * a * ws[(size_t)p] + a * a * ss[(size_t)p]);
        if (fnew - hfold[(size_t)p] <= 0.01 * a * gs[(size_t)p]) ls[(size_t)p] = 0;  // accepted
        else step[(size_t)p] = a * 0.5;
      }
    }
    for (int p = 0; p < P; ++p)
      if (ls[(size_t)p]) { step[(size_t)p] = 0.0; done[(size_t)p] = 1; }  // no descent within 30 halvings: numerically at the optimum
    GNX_HIPRET(push(step, sc3));
    hipLaunchKernelGGL(k_tr_vec<V_AXPY>, dim3(P), dim3(256), 0, st, ldw, w, s, nullptr, sc3, nullptr, nullptr, 1.0);
    forward(w, Z);  // exact Z for the new w (no drift from accumulating alpha * Zs)
    GNX_HIPRET(eval_grad());
    for (int p = 0; p < P; ++p)
      if (hact[(size_t)p] && std::fabs(hfold[(size_t)p] - hf[(size_t)p]) <= 1e-15 * std::fabs(hf[(size_t)p])) done[(size_t)p] = 1;
  }
  // ---- results ----
  std::vector<double> hw(PV);
  GNX_HIPRET(hipMemcpyAsync(hw.data(), w, PV * sizeof(double), hipMemcpyDeviceToHost, st));
  GNX_HIPRET(hipStreamSynchronize(st));
  double worst = 0.0;
  for (int p = 0; p < P; ++p)
    if (gnorm0[(size_t)p] > 0) worst = std::max(worst, std::sqrt(h2[(size_t)p]) / gnorm0[(size_t)p]);
  for (int wi = 0; wi < W; ++wi) {
    const int len = (wi == W - 1) ? g.len_last : g.len;
    for (int a = 0; a < A; ++a) {
      // A == 2: sklearn keeps ONE row (positive class 1); the kernel's one-vs-rest form takes the rows (-w, +w) (convert.py)
      const int p = (npw == 1) ? 0 : a;
      const double sgn = (npw == 1 && a == 0) ? -1.0 : 1.0;
      const double* src = hw.data() + ((size_t)wi * npw + p) * ldw;
      double* dst = h_coef + ((size_t)wi * A + a) * (size_t)ldc;
      for (int k = 0; k < len; ++k) dst[k] = sgn * src[k];
      for (int64_t k = len; k < ldc; ++k) dst[k] = 0.0;
      h_icpt[(size_t)wi * A + a] = sgn * src[ldw - 1];
    }
  }
  if (info) {
    info->newton_iterations = newton;
    info->cg_iterations = cg_total;
    info->n_problems = P;
    info->worst_rel_gradient = worst;
    double fs = 0.0;
    for (int p = 0; p < P; ++p) fs += hf[(size_t)p];
    info->objective_sum = fs;
  }
  return hipGetLastError();
}
