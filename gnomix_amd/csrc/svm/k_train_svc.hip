// k_train_svc.hip — fitting the CovRSK string-kernel SVC base (mode "best") on gfx950.
//
// Replaces CovRSKBase.train (reference src/Base/base.py:104-127 with src/Base/models.py:195-215): per window
//   SVC(kernel=CovRSK, probability=True).fit(Xw, yw)
// which is sklearn's libsvm (sklearn/svm/src/libsvm/svm.cpp, third-party) on the window's Gram matrix: one C-SVC per class
// pair, each preceded by Platt's 5-fold cross-validation (svm_binary_svc_probability) whose fold models are C-SVCs too.
//
// Passes:
//  * k_svc_pack: X int8 {0,1,2} -> per (window, row) two bit-planes of the window's SNPs over the reflect-padded coordinate
//    (base.py:41-44, windows as train_vectorized slices them; the last one is M_ + rem wide).
//  * k_svc_gram: K_w = CovRSK(Xw, Xw), upper triangle, mirrored.  Symbol equality of 32 SNPs is ~((xl^yl)|(xh^yh)); maximal
//    runs of equal symbols are peeled with ctz and each adds g(L) = sum_{m in Ms, m <= L} (L - m + 1) from an LDS table.
//    Values are exact integers below 2^24 (checked on the host from g(width)), so the float Gram equals libsvm's Qfloat
//    and its double diagonal QD.
//  * k_svc_gram_poly (GNX_SVC_KERNEL_POLY, PolynomialStringKernelBase): the same planes and Gram layout; the value of a pair is
//    (long long)(np.sum(run_value[run lengths]) / p) in numpy's summation order, again an exact integer below 2^24.
//  * k_svc_smo: one wave per solve (a class pair's full problem or one of its fold problems, any window of the batch).
//    libsvm's Solver::Solve for C-SVC (C = 1, eps = 1e-3, shrinking, no iteration cap beyond a hang guard) restated:
//    WSS3 second-order working-set selection with libsvm's tie rules (`>=` / `<=`: the LAST index wins, so the parallel
//    (value, index) reductions prefer the larger index on ties), the gradient update in double, shrinking every min(l, 1000)
//    iterations with swap_index (an explicit position -> element map), the one-time unshrink at eps * 10 and
//    reconstruct_gradient with every element summed in libsvm's order.  G, G_bar, alpha, status, y and the map live in
//    global memory (L2-resident at these sizes); Q columns are read straight from the window's Gram.
//  * k_svc_heldout: decision values of the held-out rows under their fold model, in svm_predict_values' order.
//  * GNX_SVC_KERNEL_RBF (SVMBase, src/Base/models.py:148-159: SVC(C=100., gamma=0.001, probability=True)): the Gram pass is
//    k_base_rbf.hip's (|x - y|^2 on the int8 matrix cores, Q = (float) T[d2] with T = the host's exp(-gamma k): libsvm's Qfloat of
//    the double kernel value, QD = 1); the solver is the same with C a parameter; the held-out decision values take the DOUBLE
//    kernel value T[d2] (svm_predict_values calls k_function, not Q).
//  * k_svc_sigmoid: sigmoid_train (Newton with backtracking, 100 iterations), one thread per (window, pair).
// The fold permutations (mt19937 + sklearn's Lemire bounded_rand_int) and the model assembly in sklearn's layout are host work.
//
// The restated parts of libsvm carry its licence:
//   Copyright (c) 2000-2014 Chih-Chung Chang and Chih-Jen Lin.  All rights reserved.
//   Redistribution and use in source and binary forms, with or without modification, are permitted provided that the
//   following conditions are met: 1. Redistributions of source code must retain the above copyright notice, this list of
//   conditions and the following disclaimer.  2. Redistributions in binary form must reproduce the above copyright notice, this
//   list of conditions and the following disclaimer in the documentation and/or other materials provided with the
//   distribution.  3. Neither name of copyright holders nor the names of its contributors may be used to endorse or promote
//   products derived from this software without specific prior written permission.
//   THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES,
//   INCLUDING, BUT NOT LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE
//   DISCLAIMED.  IN NO EVENT SHALL THE REGENTS OR CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL,
//   EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING, BUT NOT LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF
//   USE, DATA, OR PROFITS; OR BUSINESS INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT
//   LIABILITY, OR TORT (INCLUDING NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED
//   OF THE POSSIBILITY OF SUCH DAMAGE.
#include "../gnx_internal.h"
#include "gnx_svc_rbf.h"
#include "../gnx_window.h"
#include "gnx_np_pairwise.h"

#include <cmath>
#include <random>

namespace {

constexpr int SVC_MAX_WIDTH = 16384;          // g table in LDS: (width + 1) * 4 bytes
// The polynomial kernel's run values are doubles: (width + 1) * 8 bytes.  Its budget is the 64 KiB a block gets without asking
// for more, which also leaves room for two blocks on a CU's 160 KiB: the pass is bound by the latency of dependent LDS lookups,
// so resident waves are what it runs on.
constexpr int SVC_POLY_LDS_BUDGET = 64 * 1024;
constexpr int SVC_POLY_MAX_WIDTH = SVC_POLY_LDS_BUDGET / 8 - 1;  // 8191 SNPs
constexpr int SVC_FOLDS = 5;                  // svm_binary_svc_probability
constexpr int SVC_MAX_BATCH = 256;            // windows per batch (grid z, per-element workspace)
constexpr double SVC_EPS = 1e-3;              // sklearn SVC(tol=1e-3)
constexpr double SVC_TAU = 1e-12;             // libsvm TAU
constexpr int64_t SVC_ITER_GUARD = 50000000;  // a hang guard, not libsvm's max_iter (sklearn passes -1): counted in the info
constexpr int8_t ST_LOWER = 0, ST_UPPER = 1, ST_FREE = 2;

// one thread = one 32-SNP word of one (window, row): planes[((wl * N + n) * 2 + plane) * nwm + word]
__global__ __launch_bounds__(256) void k_svc_pack(const int8_t* X, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t ctx,
                                                   int w_first, int wb, int W, int rem, int nwm, uint32_t* planes) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)wb * N * nwm) return;
  const int wd = (int)(idx % nwm);
  const int64_t n = (idx / nwm) % N;
  const int wl = (int)(idx / ((int64_t)nwm * N));
  const int w = w_first + wl;
  const int width = (int)(M + 2 * ctx) + (w == W - 1 ? rem : 0);
  const int8_t* x = X + n * ldx;
  uint32_t lo = 0, hi = 0;
  for (int b = 0; b < 32; ++b) {
    const int t = wd * 32 + b;
    if (t < width) {
      const uint32_t v = (uint32_t)(uint8_t)x[gnx_pad_src((int64_t)w * M + t, C, ctx)];
      lo |= (v & 1u) << b;
      hi |= ((v >> 1) & 1u) << b;
    }
  }
  uint32_t* o = planes + (((int64_t)wl * N + n) * 2) * nwm;
  o[wd] = lo;
  o[nwm + wd] = hi;
}

// 16 x 16 tile of (i, j) pairs of window blockIdx.z; tiles wholly below the diagonal return at once
__global__ __launch_bounds__(256) void k_svc_gram(const uint32_t* planes, int64_t N, int nwm, int w_first, int W, int width_main,
                                                   int width_last, const uint32_t* gtab, float* gram) {
  extern __shared__ uint32_t g_lds[];
  const int wl = blockIdx.z;
  const int w = w_first + wl;
  const int width = (w == W - 1) ? width_last : width_main;
  if (blockIdx.y < blockIdx.x) return;  // block-uniform: every column index < every row index
  for (int t = threadIdx.x; t <= width; t += blockDim.x) g_lds[t] = gtab[t];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const int64_t j = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= N || j >= N || j < i) return;
  const int NW = (width + 31) >> 5;
  const uint32_t tail_mask = (width & 31) ? ((1u << (width & 31)) - 1u) : 0xffffffffu;
  const uint32_t* xi = planes + (((int64_t)wl * N + i) * 2) * nwm;
  const uint32_t* xj = planes + (((int64_t)wl * N + j) * 2) * nwm;
  uint32_t K = 0, run = 0;
  for (int q = 0; q < NW; ++q) {
    uint32_t e = ~((xi[q] ^ xj[q]) | (xi[nwm + q] ^ xj[nwm + q]));
    if (q == NW - 1) e &= tail_mask;
    if (e == 0xffffffffu) { run += 32; continue; }
    const uint32_t t = (uint32_t)__builtin_ctz(~e);  // trailing ones continue the carried run
    run += t;
    K += g_lds[run];
    run = 0;
    e >>= t;
    uint32_t remb = 32 - t;
    while (e) {
      const uint32_t z = (uint32_t)__builtin_ctz(e);
      e >>= z;
      remb -= z;
      const uint32_t o = (uint32_t)__builtin_ctz(~e);  // e has zeros above bit remb-1, so o <= remb
      if (o == remb) { run = o; break; }                // the run touches the end of the word: carry
      K += g_lds[o];
      e >>= o;
      remb -= o;
    }
  }
  K += g_lds[run];
  float* G = gram + (size_t)wl * N * N;
  G[i * N + j] = (float)K;
  G[j * N + i] = (float)K;
}

// The polynomial string kernel (PolynomialStringKernelBase, string_kernel.py:40-61): K = (long long)(np.sum(contigs ** p) / p),
// contigs = the length of the run of equal SNPs before every mismatch plus the run the window ends with (zero-length runs count).
// Same tiling and output as k_svc_gram; the run values (width + 1 doubles, the host's np.arange(width + 1) ** p) sit in LDS and are
// added in numpy's pairwise order (gnx_np_pairwise.h), so the truncated value is the reference's.  Two sweeps over the pair's words:
// the first counts the elements (the order depends on the count), the second streams them.
__global__ __launch_bounds__(256) void k_svc_gram_poly(const uint32_t* planes, int64_t N, int nwm, int w_first, int W, int width_main,
                                                        int width_last, const double* run_value, double poly_p, float* gram) {
  extern __shared__ double rv_lds[];
  const int wl = blockIdx.z;
  const int w = w_first + wl;
  const int width = (w == W - 1) ? width_last : width_main;
  if (blockIdx.y < blockIdx.x) return;  // block-uniform: every column index < every row index
  for (int t = threadIdx.x; t <= width; t += blockDim.x) rv_lds[t] = run_value[t];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const int64_t j = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= N || j >= N || j < i) return;
  const int NW = (width + 31) >> 5;
  const int tail_bits = (width & 31) ? (width & 31) : 32;
  const uint32_t tail_mask = (width & 31) ? ((1u << (width & 31)) - 1u) : 0xffffffffu;
  const uint32_t* xi = planes + (((int64_t)wl * N + i) * 2) * nwm;
  const uint32_t* xj = planes + (((int64_t)wl * N + j) * 2) * nwm;
  auto mismatches = [&](int q) -> uint32_t {  // bit t: SNP 32 q + t differs (bits past the window are clear)
    const uint32_t d = (xi[q] ^ xj[q]) | (xi[nwm + q] ^ xj[nwm + q]);
    return q == NW - 1 ? (d & tail_mask) : d;
  };
  int n_el = 1;
  for (int q = 0; q < NW; ++q) n_el += __builtin_popcount(mismatches(q));
  // generator: the word in hand is q, its mismatches from bit b on are mm (shifted down), run is the length of the open run
  int q = -1, b = 0, bits = 0, run = 0;
  uint32_t mm = 0;
  auto next_val = [&]() -> double {
    while (mm == 0u) {
      run += bits - b;  // the rest of the word matches
      if (++q == NW) { q = NW - 1; b = bits; return rv_lds[run]; }  // the run the window ends with (the last element)
      mm = mismatches(q);
      bits = (q == NW - 1) ? tail_bits : 32;
      b = 0;
    }
    const int z = __builtin_ctz(mm);
    const double v = rv_lds[run + z];
    run = 0;
    mm = (mm >> z) >> 1;
    b += z + 1;
    return v;
  };
  const double S = gnx_np_pairwise_sum(n_el, next_val);
  const float K = (float)(long long)(S / poly_p);  // numpy float -> int assignment truncates toward zero; < 2^24 (host check)
  float* G = gram + (size_t)wl * N * N;
  G[i * N + j] = K;
  G[j * N + i] = K;
}

struct SvcSolve {
  int64_t gram;  // element offset of the window's Gram in the batch buffer
  int64_t off;   // offset of this solve's elements in the per-element arrays
  int32_t l;
  int32_t reserved;
};

struct SmoArgs {
  const SvcSolve* solves;
  const float* gram;
  int64_t N;
  const int32_t* rows;   // element -> row of the window (solve order)
  const int8_t* ysg;     // element -> +1 / -1 (solve order)
  double* G;             // position-indexed working arrays
  double* Gb;
  double* al;
  int32_t* as;           // position -> element (libsvm's active_set)
  int8_t* yv;            // position -> y
  int8_t* st;            // position -> alpha status
  double* alpha_out;     // element -> alpha * y (solve_c_svc's output)
  double* rho;           // per solve
  int32_t* iters;        // per solve
  int32_t* guard;        // per solve: 1 = stopped by the hang guard or a non-finite rho
  double C;              // libsvm's cost Cp = Cn (1 for CovRSKBase, 100 for SVMBase; the fold models get the same through `weight`)
};

// (value, index) reductions over one wave: ties go to the larger index, as libsvm's sequential `>=` / `<=` scans
__device__ __forceinline__ void wave_max_last(double& v, int& i) {
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(v, o);
    const int i2 = __shfl_xor(i, o);
    if (v2 > v || (v2 == v && i2 > i)) { v = v2; i = i2; }
  }
}
__device__ __forceinline__ void wave_min_last(double& v, int& i) {
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(v, o);
    const int i2 = __shfl_xor(i, o);
    if (v2 < v || (v2 == v && i2 > i)) { v = v2; i = i2; }
  }
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

struct SmoView {
  const float* K;  // the window's Gram (N x N)
  int64_t N;
  const int32_t* rows;
  double *G, *Gb, *al;
  int32_t* as;
  int8_t *yv, *st;
  __device__ __forceinline__ int64_t row_of(int t) const { return rows[as[t]]; }
  __device__ __forceinline__ double QD(int t) const { const int64_t r = row_of(t); return (double)K[r * N + r]; }
  // SVC_Q::get_Q: (Qfloat)(y_a * y_b * kernel(a, b))
  __device__ __forceinline__ float Q(int a, int b) const {
    return (float)((double)(yv[a] * yv[b]) * (double)K[row_of(a) * N + row_of(b)]);
  }
};

__device__ void smo_swap(const SmoView& v, int i, int j) {
  { const double t = v.G[i]; v.G[i] = v.G[j]; v.G[j] = t; }
  { const double t = v.Gb[i]; v.Gb[i] = v.Gb[j]; v.Gb[j] = t; }
  { const double t = v.al[i]; v.al[i] = v.al[j]; v.al[j] = t; }
  { const int32_t t = v.as[i]; v.as[i] = v.as[j]; v.as[j] = t; }
  { const int8_t t = v.yv[i]; v.yv[i] = v.yv[j]; v.yv[j] = t; }
  { const int8_t t = v.st[i]; v.st[i] = v.st[j]; v.st[j] = t; }
}

// Solver::reconstruct_gradient (p = -1): every inactive G[j] = G_bar[j] - 1 + sum over free positions f (ascending) of
// alpha[f] * Q_f[j], one element per lane; both of libsvm's loop orders add the same products to an element in this order
__device__ void smo_reconstruct(const SmoView& v, int l, int active) {
  if (active == l) return;
  for (int j = active + (int)threadIdx.x; j < l; j += 64) {
    double g = v.Gb[j] + -1.0;
    for (int f = 0; f < active; ++f)
      if (v.st[f] == ST_FREE) g += v.al[f] * (double)v.Q(f, j);
    v.G[j] = g;
  }
  __syncthreads();
}

__device__ __forceinline__ bool be_shrunk(const SmoView& v, int i, double Gmax1, double Gmax2) {
  if (v.st[i] == ST_UPPER) return v.yv[i] == 1 ? (-v.G[i] > Gmax1) : (-v.G[i] > Gmax2);
  if (v.st[i] == ST_LOWER) return v.yv[i] == 1 ? (v.G[i] > Gmax2) : (v.G[i] > Gmax1);
  return false;
}

// Solver::select_working_set -> 1 when optimal
__device__ int smo_select(const SmoView& v, int active, int& out_i, int& out_j) {
  const int lane = threadIdx.x;
  double Gmax = -INFINITY;
  int Gmax_idx = -1;
  for (int t = lane; t < active; t += 64) {
    const bool pos = v.yv[t] == 1;
    const bool ok = pos ? v.st[t] != ST_UPPER : v.st[t] != ST_LOWER;
    const double c = pos ? -v.G[t] : v.G[t];
    if (ok && c >= Gmax) { Gmax = c; Gmax_idx = t; }
  }
  wave_max_last(Gmax, Gmax_idx);
  const int i = Gmax_idx;
  double Gmax2 = -INFINITY, obj_min = INFINITY;
  int Gmin_idx = -1;
  const double QDi = i != -1 ? v.QD(i) : 0.0;
  const int yi = i != -1 ? v.yv[i] : 0;
  for (int j = lane; j < active; j += 64) {
    const bool pos = v.yv[j] == 1;
    if (pos ? (v.st[j] == ST_LOWER) : (v.st[j] == ST_UPPER)) continue;
    const double Gj = v.G[j];
    const double grad_diff = pos ? Gmax + Gj : Gmax - Gj;
    const double m2 = pos ? Gj : -Gj;
    if (m2 >= Gmax2) Gmax2 = m2;
    if (grad_diff > 0) {  // never true when i == -1 (Gmax = -inf): Q_i is not read then, as in libsvm
      const double qij = (double)v.Q(i, j);
      const double quad_coef = pos ? QDi + v.QD(j) - 2.0 * yi * qij : QDi + v.QD(j) + 2.0 * yi * qij;
      const double obj_diff = quad_coef > 0 ? -(grad_diff * grad_diff) / quad_coef : -(grad_diff * grad_diff) / SVC_TAU;
      if (obj_diff <= obj_min) { obj_min = obj_diff; Gmin_idx = j; }
    }
  }
  Gmax2 = wave_max(Gmax2);
  wave_min_last(obj_min, Gmin_idx);
  if (Gmax + Gmax2 < SVC_EPS || Gmin_idx == -1) return 1;
  out_i = i;
  out_j = Gmin_idx;
  return 0;
}

__global__ __launch_bounds__(64) void k_svc_smo(SmoArgs a) {
  __shared__ int sh_active;
  const int lane = threadIdx.x;
  const SvcSolve s = a.solves[blockIdx.x];
  const int l = s.l;
  SmoView v;
  v.K = a.gram + s.gram;
  v.N = a.N;
  v.rows = a.rows + s.off;
  v.G = a.G + s.off; v.Gb = a.Gb + s.off; v.al = a.al + s.off;
  v.as = a.as + s.off; v.yv = a.yv + s.off; v.st = a.st + s.off;
  const int8_t* y0 = a.ysg + s.off;
  for (int t = lane; t < l; t += 64) {
    v.G[t] = -1.0;  // p = minus ones; every alpha starts at 0 = lower bound, so G_bar = 0 and no Q row enters the start
    v.Gb[t] = 0.0;
    v.al[t] = 0.0;
    v.as[t] = t;
    v.yv[t] = y0[t];
    v.st[t] = ST_LOWER;
  }
  __syncthreads();

  int active = l, counter = (l < 1000 ? l : 1000) + 1, guard = 0;
  bool unshrink = false;
  int64_t iter = 0;
  while (true) {
    if (iter >= SVC_ITER_GUARD) { guard = 1; break; }
    if (--counter == 0) {
      counter = l < 1000 ? l : 1000;
      // ---- do_shrinking ----
      double Gmax1 = -INFINITY, Gmax2 = -INFINITY;
      for (int t = lane; t < active; t += 64) {
        const double g = v.G[t];
        if (v.yv[t] == 1) {
          if (v.st[t] != ST_UPPER) Gmax1 = fmax(Gmax1, -g);
          if (v.st[t] != ST_LOWER) Gmax2 = fmax(Gmax2, g);
        } else {
          if (v.st[t] != ST_UPPER) Gmax2 = fmax(Gmax2, -g);
          if (v.st[t] != ST_LOWER) Gmax1 = fmax(Gmax1, g);
        }
      }
      Gmax1 = wave_max(Gmax1);
      Gmax2 = wave_max(Gmax2);
      if (!unshrink && Gmax1 + Gmax2 <= SVC_EPS * 10) {
        unshrink = true;
        smo_reconstruct(v, l, active);
        active = l;
      }
      if (lane == 0) {  // the sequential shrink walk: its swaps decide later positions (and so later tie-breaks)
        int act = active;
        for (int i = 0; i < act; ++i)
          if (be_shrunk(v, i, Gmax1, Gmax2)) {
            act--;
            while (act > i) {
              if (!be_shrunk(v, act, Gmax1, Gmax2)) { smo_swap(v, i, act); break; }
              act--;
            }
          }
        sh_active = act;
      }
      __syncthreads();
      active = sh_active;
      __syncthreads();
    }
    int i = -1, j = -1;
    if (smo_select(v, active, i, j) != 0) {
      smo_reconstruct(v, l, active);
      active = l;
      if (smo_select(v, active, i, j) != 0) break;
      counter = 1;  // do shrinking next iteration
    }
    ++iter;

    // ---- update alpha[i], alpha[j] (every lane computes the same values) ----
    const double C_i = a.C, C_j = a.C;
    const double Qij = (double)v.Q(i, j);
    const double QDi = v.QD(i), QDj = v.QD(j);
    const double Gi = v.G[i], Gj = v.G[j];
    const double old_ai = v.al[i], old_aj = v.al[j];
    const int yi = v.yv[i], yj = v.yv[j];
    const int8_t sti = v.st[i], stj = v.st[j];
    double ai = old_ai, aj = old_aj;
    if (yi != yj) {
      double quad_coef = QDi + QDj + 2 * Qij;
      if (quad_coef <= 0) quad_coef = SVC_TAU;
      const double delta = (-Gi - Gj) / quad_coef;
      const double diff = ai - aj;
      ai += delta;
      aj += delta;
      if (diff > 0) {
        if (aj < 0) { aj = 0; ai = diff; }
      } else {
        if (ai < 0) { ai = 0; aj = -diff; }
      }
      if (diff > C_i - C_j) {
        if (ai > C_i) { ai = C_i; aj = C_i - diff; }
      } else {
        if (aj > C_j) { aj = C_j; ai = C_j + diff; }
      }
    } else {
      double quad_coef = QDi + QDj - 2 * Qij;
      if (quad_coef <= 0) quad_coef = SVC_TAU;
      const double delta = (Gi - Gj) / quad_coef;
      const double sum = ai + aj;
      ai -= delta;
      aj += delta;
      if (sum > C_i) {
        if (ai > C_i) { ai = C_i; aj = sum - C_i; }
      } else {
        if (aj < 0) { aj = 0; ai = sum; }
      }
      if (sum > C_j) {
        if (aj > C_j) { aj = C_j; ai = sum - C_j; }
      } else {
        if (ai < 0) { ai = 0; aj = sum; }
      }
    }
    const double dai = ai - old_ai, daj = aj - old_aj;
    __syncthreads();  // every lane has read G[i], G[j], alpha and status before they change
    // ---- update G over the active set ----
    for (int k = lane; k < active; k += 64) v.G[k] += (double)v.Q(i, k) * dai + (double)v.Q(j, k) * daj;
    // ---- alpha status and G_bar ----
    const int8_t nsti = ai >= C_i ? ST_UPPER : (ai <= 0 ? ST_LOWER : ST_FREE);
    const int8_t nstj = aj >= C_j ? ST_UPPER : (aj <= 0 ? ST_LOWER : ST_FREE);
    const bool ui = sti == ST_UPPER, uj = stj == ST_UPPER;
    if (ui != (nsti == ST_UPPER)) {
      for (int k = lane; k < l; k += 64) {
        const double q = (double)v.Q(i, k);
        if (ui) v.Gb[k] -= C_i * q; else v.Gb[k] += C_i * q;
      }
    }
    if (uj != (nstj == ST_UPPER)) {  // same lane -> same k as the loop above: each element gets i's term, then j's
      for (int k = lane; k < l; k += 64) {
        const double q = (double)v.Q(j, k);
        if (uj) v.Gb[k] -= C_j * q; else v.Gb[k] += C_j * q;
      }
    }
    __syncthreads();
    if (lane == 0) {
      v.al[i] = ai; v.al[j] = aj;
      v.st[i] = nsti; v.st[j] = nstj;
    }
    __syncthreads();
  }

  // ---- calculate_rho (sequential sum), put back the solution ----
  if (lane == 0) {
    int nr_free = 0;
    double ub = INFINITY, lb = -INFINITY, sum_free = 0;
    for (int i = 0; i < active; ++i) {
      const double yG = v.yv[i] * v.G[i];
      if (v.st[i] == ST_UPPER) {
        if (v.yv[i] == -1) ub = fmin(ub, yG); else lb = fmax(lb, yG);
      } else if (v.st[i] == ST_LOWER) {
        if (v.yv[i] == 1) ub = fmin(ub, yG); else lb = fmax(lb, yG);
      } else {
        ++nr_free;
        sum_free += yG;
      }
    }
    const double r = nr_free > 0 ? sum_free / nr_free : (ub + lb) / 2;
    a.rho[blockIdx.x] = r;
    a.iters[blockIdx.x] = (int32_t)(iter < INT32_MAX ? iter : INT32_MAX);
    a.guard[blockIdx.x] = guard | (isfinite(r) ? 0 : 1);
  }
  for (int t = lane; t < l; t += 64) {
    const int e = v.as[t];
    a.alpha_out[s.off + e] = v.al[t] * y0[e];
  }
}

// held-out decision values: task t = (fold solve, window row, destination); sum over the fold model's support vectors in its
// regrouped order (svm_predict_values: class 0 then class 1), minus rho, times submodel->label[0] = -1
__global__ __launch_bounds__(256) void k_svc_heldout(const SvcSolve* solves, const float* gram, int64_t N, const int32_t* rows,
                                                      const double* alpha_out, const double* rho, int64_t n_tasks,
                                                      const int32_t* t_solve, const int32_t* t_row, const int64_t* t_dst, double* decv,
                                                      const int32_t* d2, const double* tab) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  const SvcSolve s = solves[t_solve[t]];
  const float* Kx = gram + s.gram + (int64_t)t_row[t] * N;
  double sum = 0;
  if (d2) {  // RBF: k_function's double kernel value, not the float Q
    const int32_t* Dx = d2 + s.gram + (int64_t)t_row[t] * N;
    for (int e = 0; e < s.l; ++e) {
      const double c = alpha_out[s.off + e];
      if (fabs(c) > 0) sum += c * tab[Dx[rows[s.off + e]]];
    }
  } else {
    for (int e = 0; e < s.l; ++e) {
      const double c = alpha_out[s.off + e];
      if (fabs(c) > 0) sum += c * (double)Kx[rows[s.off + e]];
    }
  }
  sum -= rho[t_solve[t]];
  decv[t_dst[t]] = sum * -1;
}

// sigmoid_train per (window, pair): decision values of the pair's l rows in pair order (class i rows are +1, then class j rows)
__global__ __launch_bounds__(64) void k_svc_sigmoid(int n_pairs, const int64_t* dec_off, const int32_t* pl, const int32_t* pci,
                                                     const double* decv, double* probA, double* probB) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int l = pl[p], ci = pci[p];
  const double* dec = decv + dec_off[p];
  const double prior1 = (double)ci, prior0 = (double)(l - ci);
  const int max_iter = 100;
  const double min_step = 1e-10, sigma = 1e-12, eps = 1e-5;
  const double hiTarget = (prior1 + 1.0) / (prior1 + 2.0);
  const double loTarget = 1 / (prior0 + 2.0);
  double A = 0.0, B = log((prior0 + 1.0) / (prior1 + 1.0));
  double fval = 0.0;
  for (int i = 0; i < l; ++i) {
    const double t = i < ci ? hiTarget : loTarget;
    const double fApB = dec[i] * A + B;
    if (fApB >= 0) fval += t * fApB + log(1 + exp(-fApB));
    else fval += (t - 1) * fApB + log(1 + exp(fApB));
  }
  for (int iter = 0; iter < max_iter; ++iter) {
    double h11 = sigma, h22 = sigma, h21 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int i = 0; i < l; ++i) {
      const double fApB = dec[i] * A + B;
      double pp, q;
      if (fApB >= 0) {
        pp = exp(-fApB) / (1.0 + exp(-fApB));
        q = 1.0 / (1.0 + exp(-fApB));
      } else {
        pp = 1.0 / (1.0 + exp(fApB));
        q = exp(fApB) / (1.0 + exp(fApB));
      }
      const double d2 = pp * q;
      h11 += dec[i] * dec[i] * d2;
      h22 += d2;
      h21 += dec[i] * d2;
      const double d1 = (i < ci ? hiTarget : loTarget) - pp;
      g1 += dec[i] * d1;
      g2 += d1;
    }
    if (fabs(g1) < eps && fabs(g2) < eps) break;
    const double det = h11 * h22 - h21 * h21;
    const double dA = -(h22 * g1 - h21 * g2) / det;
    const double dB = -(-h21 * g1 + h11 * g2) / det;
    const double gd = g1 * dA + g2 * dB;
    double stepsize = 1;
    while (stepsize >= min_step) {
      const double newA = A + stepsize * dA, newB = B + stepsize * dB;
      double newf = 0.0;
      for (int i = 0; i < l; ++i) {
        const double t = i < ci ? hiTarget : loTarget;
        const double fApB = dec[i] * newA + newB;
        if (fApB >= 0) newf += t * fApB + log(1 + exp(-fApB));
        else newf += (t - 1) * fApB + log(1 + exp(fApB));
      }
      if (newf < fval + 0.0001 * stepsize * gd) {
        A = newA; B = newB; fval = newf;
        break;
      }
      stepsize = stepsize / 2.0;
    }
    if (stepsize < min_step) break;
  }
  probA[p] = A;
  probB[p] = B;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

// numpy's legacy RandomState(seed).random_sample(): MT19937 (init_genrand, as std::mt19937) + genrand_res53
std::vector<int32_t> cov_sample(int width, uint32_t seed = 37, double alpha = 0.6, double beta = 1.0) {
  std::mt19937 mt(seed);
  std::vector<int32_t> ms{1};
  for (int m = 2; m <= width; ++m) {
    const uint32_t a = mt() >> 5, b = mt() >> 6;
    const double u = (a * 67108864.0 + b) / 9007199254740992.0;
    if ((1 - std::pow(alpha, (double)(m - ms.back() + 1))) * std::pow((double)m, -beta) >= u) ms.push_back(m);
  }
  return ms;
}

std::vector<int32_t> kernel_lengths(int32_t kernel_kind, int width) {
  if (kernel_kind == GNX_SVC_KERNEL_SUBSTRINGS) return cov_sample(width);
  std::vector<int32_t> ms;
  for (int m = 1; m <= width; ++m) ms.push_back(m);
  return ms;
}

// g(L) over the kernel's lengths (prefix-stable in the width: one table serves both widths); < 2^24: svc_kernel_check bounds g(width)
std::vector<uint32_t> run_table(int32_t kernel_kind, int width) {
  const std::vector<int32_t> ms = kernel_lengths(kernel_kind, width);
  std::vector<uint32_t> g(width + 1, 0);
  for (int L = 1; L <= width; ++L) {
    uint64_t s = 0;
    for (int32_t m : ms)
      if (m <= L) s += (uint64_t)(L - m + 1);
    g[L] = (uint32_t)s;
  }
  return g;
}

struct SvcPoly {  // GNX_SVC_KERNEL_POLY: the exponent and the caller's (host) table np.arange(n) ** p
  double p;
  const double* run_value;
  int64_t n;
};

// the string kernels' Gram pass of one batch of windows: k_svc_pack, then k_svc_gram (g table) or k_svc_gram_poly (run values)
struct GramPass {
  int64_t N;
  int nwm, W, width_main, width_last;
  const uint32_t* dg;  // device, width_last + 1 (the integer kernels)
  const double* drv;   // device, width_last + 1 (the polynomial kernel), or NULL
  double poly_p;
  size_t lds() const { return (size_t)(width_last + 1) * (drv ? 8 : 4); }
};

hipError_t gram_pass_prepare(const GramPass& gp) {
  if (!gp.drv && gp.lds() > 64 * 1024)  // (the polynomial kernel's table stays within SVC_POLY_LDS_BUDGET)
    return hipFuncSetAttribute((const void*)k_svc_gram, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gp.lds());
  return hipSuccess;
}

hipError_t gram_pass(const GramPass& gp, const int8_t* dX, int64_t ldx, int64_t C, int64_t M, int64_t cx, int w0, int nb, uint32_t* dPl,
                     float* dGram, hipStream_t s) {
  const int64_t n_words = (int64_t)nb * gp.N * gp.nwm;
  hipLaunchKernelGGL(k_svc_pack, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, s, dX, gp.N, ldx, C, M, cx, w0, nb, gp.W,
                     (int)(C % M), gp.nwm, dPl);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned tiles = (unsigned)((gp.N + 15) / 16);
  if (gp.drv)
    hipLaunchKernelGGL(k_svc_gram_poly, dim3(tiles, tiles, (unsigned)nb), dim3(256), gp.lds(), s, dPl, gp.N, gp.nwm, w0, gp.W, gp.width_main,
                       gp.width_last, gp.drv, gp.poly_p, dGram);
  else
    hipLaunchKernelGGL(k_svc_gram, dim3(tiles, tiles, (unsigned)nb), dim3(256), gp.lds(), s, dPl, gp.N, gp.nwm, w0, gp.W, gp.width_main,
                       gp.width_last, gp.dg, dGram);
  return hipGetLastError();
}

// sklearn's newrand.h: mt19937 + the tweaked Lemire post-processor
uint32_t bounded_rand_int(std::mt19937& mt, uint32_t range) {
  uint32_t x = mt();
  uint64_t m = uint64_t(x) * uint64_t(range);
  uint32_t l = uint32_t(m);
  if (l < range) {
    uint32_t t = -range;
    if (t >= range) {
      t -= range;
      if (t >= range) t %= range;
    }
    while (l < t) {
      x = mt();
      m = uint64_t(x) * uint64_t(range);
      l = uint32_t(m);
    }
  }
  return (uint32_t)(m >> 32);
}

// svm_binary_svc_probability's shuffle: every pair's draws start from a freshly seeded generator (svm_train seeds it, and each
// fold's nested svm_train seeds it again before the next pair shuffles)
void fold_permutation(uint32_t seed, int l, int32_t* perm) {
  std::mt19937 mt(seed);
  for (int i = 0; i < l; ++i) perm[i] = i;
  for (int i = 0; i < l; ++i) {
    const int j = i + (int)bounded_rand_int(mt, (uint32_t)(l - i));
    std::swap(perm[i], perm[j]);
  }
}

struct DevEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~DevEvents() {
    for (auto& x : e)
      if (x) (void)hipEventDestroy(x);
  }
};
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PairTask {  // one (window, class pair) of a batch
  int ci, cj, full_solve;
};

int train_svc_impl(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t cx,
                   int32_t A, const gnx_svc_params& prm, const SvcPoly* poly, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support,
                   int32_t* support, double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info) {
  const int32_t kernel_kind = prm.kernel_kind;
  const bool rbf = kernel_kind == GNX_SVC_KERNEL_RBF;
  const int W = (int)(C / M), rem = (int)(C % M), P = A * (A - 1) / 2;
  const int width_main = (int)(M + 2 * cx), width_last = width_main + rem;
  // g(L) over the kernel's lengths (prefix-stable in the width: one table serves both widths)
  const std::vector<uint32_t> g = (rbf || poly) ? std::vector<uint32_t>(width_last + 1, 0) : run_table(kernel_kind, width_last);
  const int nwm = (width_last + 31) / 32;
  // RBF: staged int8 rows (Np x kp per window) instead of bit-planes, the int32 distances beside the float Gram, one exp table
  const int64_t Np = (N + 63) / 64 * 64;
  const int kp = (width_last + 63) / 64 * 64;
  std::vector<double> tab;
  if (rbf) gnx_rbf_table(prm.gamma, gnx_rbf_table_len(width_last), tab);
  const size_t gram_w = (size_t)N * N * 4;
  // per window: every pair's full problem plus its folds' training parts: at most 5 l elements per pair, sum of l = (A - 1) N
  const size_t elems_w = (size_t)5 * (A - 1) * N;
  const size_t elem_bytes = 4 * 8 + 2 * 4 + 3;
  size_t wbs = std::min<size_t>((size_t)W, GNX_SVC_GRAM_BUDGET / (gram_w * (rbf ? 2 : 1)));
  wbs = std::min<size_t>(wbs, ((size_t)2 << 30) / (elems_w * elem_bytes));
  const int wb = (int)std::max<size_t>(1, std::min<size_t>(wbs, SVC_MAX_BATCH));

  // ---- device buffers, sized for a full batch ----
  const size_t max_solves = (size_t)wb * P * (1 + SVC_FOLDS), max_elems = (size_t)wb * elems_w;
  const size_t max_rows = (size_t)wb * (A - 1) * N, max_pairs = (size_t)wb * P;  // held-out tasks / decision values
  const size_t bXw = rbf ? up256((size_t)wb * Np * kp) : 0, bNrm = rbf ? up256((size_t)wb * Np * 4) : 0;
  const size_t bD2 = rbf ? up256((size_t)wb * gram_w) : 0, bTab = rbf ? up256(tab.size() * 8) : 0;
  const size_t bPl = rbf ? 0 : up256((size_t)wb * N * 2 * nwm * 4), bGram = up256((size_t)wb * gram_w), bG = up256((size_t)(width_last + 1) * 4);
  const size_t bRv = poly ? up256((size_t)(width_last + 1) * 8) : 0;
  const size_t bSol = up256(max_solves * sizeof(SvcSolve)), bE8 = up256(max_elems * 8), bE4 = up256(max_elems * 4), bE1 = up256(max_elems);
  const size_t bS8 = up256(max_solves * 8), bS4 = up256(max_solves * 4);
  const size_t bT4 = up256(max_rows * 4), bT8 = up256(max_rows * 8), bP8 = up256(max_pairs * 8), bP4 = up256(max_pairs * 4);
  const size_t total = bPl + bGram + bG + bSol + 4 * bE8 + 2 * bE4 + 3 * bE1 + bS8 + 2 * bS4 + 2 * bT4 + 2 * bT8 + 3 * bP8 + 2 * bP4 + bXw + bNrm + bD2 + bTab + bRv;
  gnx_dev_tmp blk;
  hipError_t e = blk.alloc(total);
  if (e != hipSuccess) {
    blk.p = nullptr;
    return gnx_fail(ctx, GNX_ENOMEM, std::string("train_svc: hipMalloc of ") + std::to_string(total >> 20) + " MiB: " + hipGetErrorString(e));
  }
  char* q = (char*)blk.p;
  auto take = [&](size_t b) { char* r = q; q += b; return r; };
  uint32_t* dPl = (uint32_t*)take(bPl);
  float* dGram = (float*)take(bGram);
  uint32_t* dg = (uint32_t*)take(bG);
  SvcSolve* dSol = (SvcSolve*)take(bSol);
  double* dGv = (double*)take(bE8);
  double* dGb = (double*)take(bE8);
  double* dAl = (double*)take(bE8);
  double* dAo = (double*)take(bE8);
  int32_t* dAs = (int32_t*)take(bE4);
  int32_t* dRows = (int32_t*)take(bE4);
  int8_t* dYv = (int8_t*)take(bE1);
  int8_t* dSt = (int8_t*)take(bE1);
  int8_t* dYs = (int8_t*)take(bE1);
  double* dRho = (double*)take(bS8);
  int32_t* dIt = (int32_t*)take(bS4);
  int32_t* dGd = (int32_t*)take(bS4);
  int32_t* dTs = (int32_t*)take(bT4);
  int32_t* dTr = (int32_t*)take(bT4);
  int64_t* dTd = (int64_t*)take(bT8);
  double* dDec = (double*)take(bT8);
  int64_t* dPoff = (int64_t*)take(bP8);
  double* dPa = (double*)take(bP8);
  double* dPb = (double*)take(bP8);
  int32_t* dPlen = (int32_t*)take(bP4);
  int32_t* dPci = (int32_t*)take(bP4);
  int8_t* dXw = (int8_t*)take(bXw);
  int32_t* dNrm = (int32_t*)take(bNrm);
  int32_t* dD2 = rbf ? (int32_t*)take(bD2) : nullptr;
  double* dTab = rbf ? (double*)take(bTab) : nullptr;
  double* dRv = poly ? (double*)take(bRv) : nullptr;

  hipStream_t s = ctx->stream;
  DevEvents ev;
  for (auto& x : ev.e) HIPCHK(ctx, hipEventCreate(&x));
  HIPCHK(ctx, hipMemcpyAsync(dg, g.data(), (size_t)(width_last + 1) * 4, hipMemcpyHostToDevice, s));
  if (rbf) HIPCHK(ctx, hipMemcpyAsync(dTab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
  if (poly) HIPCHK(ctx, hipMemcpyAsync(dRv, poly->run_value, (size_t)(width_last + 1) * 8, hipMemcpyHostToDevice, s));
  const GramPass gp{N, nwm, W, width_main, width_last, dg, dRv, poly ? poly->p : 0.0};
  if (!rbf) HIPCHK(ctx, gram_pass_prepare(gp));

  gnx_svc_train_info inf{};
  std::vector<std::vector<int32_t>> cls_rows(A);
  for (int w0 = 0; w0 < W; w0 += wb) {
    const int nb = std::min(wb, W - w0);
    // ---- host: problems, fold permutations, held-out tasks ----
    std::vector<SvcSolve> sol;
    std::vector<int32_t> rows, ts, tr, plen, pci, perm;
    std::vector<int8_t> ysg;
    std::vector<int64_t> td, poff;
    std::vector<double> dec;
    std::vector<PairTask> pairs;
    for (int wl = 0; wl < nb; ++wl) {
      const int w = w0 + wl;
      const int64_t gram_off = (int64_t)wl * N * N;
      for (auto& c : cls_rows) c.clear();
      for (int64_t n = 0; n < N; ++n) cls_rows[y[n * W + w]].push_back((int32_t)n);
      auto begin_solve = [&]() { sol.push_back(SvcSolve{gram_off, (int64_t)rows.size(), 0, 0}); return (int)sol.size() - 1; };
      auto add = [&](int sid, int32_t row, int8_t ys) { rows.push_back(row); ysg.push_back(ys); sol[sid].l++; };
      for (int ci = 0; ci < A; ++ci)
        for (int cj = ci + 1; cj < A; ++cj) {
          std::vector<int32_t> prow = cls_rows[ci];  // pair order: class ci rows (+1), then class cj rows (-1)
          prow.insert(prow.end(), cls_rows[cj].begin(), cls_rows[cj].end());
          const int l = (int)prow.size(), nci = (int)cls_rows[ci].size();
          const int64_t doff = (int64_t)dec.size();
          dec.resize(dec.size() + l, 0.0);
          perm.resize(l);
          fold_permutation(seeds[w], l, perm.data());
          for (int f = 0; f < SVC_FOLDS; ++f) {
            const int begin = f * l / SVC_FOLDS, end = (f + 1) * l / SVC_FOLDS;
            int pc = 0, nc = 0;
            for (int j = 0; j < l; ++j)
              if (j < begin || j >= end) (perm[j] < nci ? pc : nc)++;
            if (pc == 0 || nc == 0) {
              const double val = (pc == 0 && nc == 0) ? 0.0 : (pc > 0 ? 1.0 : -1.0);
              for (int j = begin; j < end; ++j) dec[doff + perm[j]] = val;
              continue;
            }
            // the nested svm_train groups its labels sorted (-1 first): the -1 rows come first and become the solver's +1
            const int sid = begin_solve();
            for (int j = 0; j < l; ++j)
              if ((j < begin || j >= end) && perm[j] >= nci) add(sid, prow[perm[j]], 1);
            for (int j = 0; j < l; ++j)
              if ((j < begin || j >= end) && perm[j] < nci) add(sid, prow[perm[j]], -1);
            for (int j = begin; j < end; ++j) {
              ts.push_back(sid);
              tr.push_back(prow[perm[j]]);
              td.push_back(doff + perm[j]);
            }
          }
          const int full = begin_solve();
          for (int k = 0; k < l; ++k) add(full, prow[k], k < nci ? 1 : -1);
          poff.push_back(doff);
          plen.push_back(l);
          pci.push_back(nci);
          pairs.push_back(PairTask{ci, cj, full});
        }
    }
    const int n_sol = (int)sol.size(), n_pairs = (int)pairs.size();
    const int64_t n_el = (int64_t)rows.size(), n_tasks = (int64_t)ts.size();
    HIPCHK(ctx, hipMemcpyAsync(dSol, sol.data(), sol.size() * sizeof(SvcSolve), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dRows, rows.data(), n_el * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dYs, ysg.data(), n_el, hipMemcpyHostToDevice, s));
    if (n_tasks) {
      HIPCHK(ctx, hipMemcpyAsync(dTs, ts.data(), n_tasks * 4, hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dTr, tr.data(), n_tasks * 4, hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dTd, td.data(), n_tasks * 8, hipMemcpyHostToDevice, s));
    }
    HIPCHK(ctx, hipMemcpyAsync(dDec, dec.data(), dec.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dPoff, poff.data(), n_pairs * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dPlen, plen.data(), n_pairs * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dPci, pci.data(), n_pairs * 4, hipMemcpyHostToDevice, s));

    // ---- Gram ----
    HIPCHK(ctx, hipEventRecord(ev.e[0], s));
    if (rbf) {
      HIPCHK(ctx, gnx_launch_rbf_stage(dX, N, ldx, C, M, cx, w0, nb, W, rem, Np, kp, dXw, dNrm, s));
      HIPCHK(ctx, gnx_launch_rbf_gram(dXw, dNrm, N, Np, kp, nb, dTab, (int32_t)tab.size() - 1, dGram, dD2, s));
    } else {
      HIPCHK(ctx, gram_pass(gp, dX, ldx, C, M, cx, w0, nb, dPl, dGram, s));
    }
    HIPCHK(ctx, hipEventRecord(ev.e[1], s));
    // ---- SMO ----
    SmoArgs sa{dSol, dGram, N, dRows, dYs, dGv, dGb, dAl, dAs, dYv, dSt, dAo, dRho, dIt, dGd, prm.C};
    hipLaunchKernelGGL(k_svc_smo, dim3((unsigned)n_sol), dim3(64), 0, s, sa);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev.e[2], s));
    // ---- Platt ----
    if (n_tasks) {
      hipLaunchKernelGGL(k_svc_heldout, dim3((unsigned)((n_tasks + 255) / 256)), dim3(256), 0, s, dSol, dGram, N, dRows, dAo, dRho, n_tasks,
                         dTs, dTr, dTd, dDec, dD2, dTab);
      HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_svc_sigmoid, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), 0, s, n_pairs, dPoff, dPlen, dPci, dDec, dPa, dPb);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev.e[3], s));

    std::vector<double> alpha(n_el), rho(n_sol), pa(n_pairs), pb(n_pairs);
    std::vector<int32_t> its(n_sol), gd(n_sol);
    HIPCHK(ctx, hipMemcpyAsync(alpha.data(), dAo, n_el * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(rho.data(), dRho, n_sol * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(its.data(), dIt, n_sol * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(gd.data(), dGd, n_sol * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pa.data(), dPa, n_pairs * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pb.data(), dPb, n_pairs * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    float t01 = 0, t12 = 0, t23 = 0;
    HIPCHK(ctx, hipEventElapsedTime(&t01, ev.e[0], ev.e[1]));
    HIPCHK(ctx, hipEventElapsedTime(&t12, ev.e[1], ev.e[2]));
    HIPCHK(ctx, hipEventElapsedTime(&t23, ev.e[2], ev.e[3]));
    inf.gram_ms += t01;
    inf.smo_ms += t12;
    inf.platt_ms += t23;
    inf.n_solves += n_sol;
    for (int k = 0; k < n_sol; ++k) {
      inf.smo_iterations += its[k];
      inf.n_guarded += gd[k];
    }

    // ---- assembly in sklearn's layout (svm_train's "build output") ----
    for (int wl = 0; wl < nb; ++wl) {
      const int w = w0 + wl;
      const PairTask* wp = &pairs[(size_t)wl * P];
      for (auto& c : cls_rows) c.clear();
      for (int64_t n = 0; n < N; ++n) cls_rows[y[n * W + w]].push_back((int32_t)n);
      std::vector<int> start(A + 1, 0);
      for (int c = 0; c < A; ++c) start[c + 1] = start[c] + (int)cls_rows[c].size();
      std::vector<char> nonzero((size_t)N, 0);  // grouped (class-major) order
      for (int p = 0; p < P; ++p) {
        const double* al = &alpha[sol[wp[p].full_solve].off];
        const int i = wp[p].ci, j = wp[p].cj, ci = (int)cls_rows[i].size(), cj = (int)cls_rows[j].size();
        for (int k = 0; k < ci; ++k) if (fabs(al[k]) > 0) nonzero[start[i] + k] = 1;
        for (int k = 0; k < cj; ++k) if (fabs(al[ci + k]) > 0) nonzero[start[j] + k] = 1;
      }
      std::vector<int> nz_start(A, 0), nz_count(A, 0);
      int total_sv = 0;
      for (int c = 0; c < A; ++c) {
        for (int k = start[c]; k < start[c + 1]; ++k) nz_count[c] += nonzero[k];
        total_sv += nz_count[c];
        n_support[(size_t)w * A + c] = nz_count[c];
        if (c) nz_start[c] = nz_start[c - 1] + nz_count[c - 1];
      }
      n_sv[w] = total_sv;
      int32_t* sup = support + (size_t)w * N;
      int o = 0;
      for (int c = 0; c < A; ++c)
        for (int k = 0; k < (int)cls_rows[c].size(); ++k)
          if (nonzero[start[c] + k]) sup[o++] = cls_rows[c][k];
      double* dc = dual_coef + (size_t)w * (A - 1) * N;
      for (int p = 0; p < P; ++p) {
        const double* al = &alpha[sol[wp[p].full_solve].off];
        const int i = wp[p].ci, j = wp[p].cj, ci = (int)cls_rows[i].size(), cj = (int)cls_rows[j].size();
        int qq = nz_start[i];
        for (int k = 0; k < ci; ++k) if (nonzero[start[i] + k]) dc[(size_t)(j - 1) * N + qq++] = al[k];
        qq = nz_start[j];
        for (int k = 0; k < cj; ++k) if (nonzero[start[j] + k]) dc[(size_t)i * N + qq++] = al[ci + k];
        const double r = rho[wp[p].full_solve];
        intercept[(size_t)w * P + p] = (r != 0) ? -r : 0;  // sklearn's copy_intercept (no -0.0)
        prob_a[(size_t)w * P + p] = pa[(size_t)wl * P + p];
        prob_b[(size_t)w * P + p] = pb[(size_t)wl * P + p];
      }
    }
  }
  if (info) *info = inf;
  return GNX_OK;
}

// what a kernel kind asks of the geometry: widths the tables fit, kernel values that are exact floats, a Gram within the budget
int svc_kernel_check(gnx_ctx* ctx, const char* who, int64_t N, int64_t C, int64_t M, int64_t cx, int32_t kernel_kind, double gamma,
                     const SvcPoly* poly) {
  const std::string pre = std::string(who) + ": ";
  const int64_t width = M + 2 * cx + C % M;
  if (kernel_kind == GNX_SVC_KERNEL_RBF) {
    if (!(gamma > 0.0) || !std::isfinite(gamma)) return gnx_fail(ctx, GNX_EINVAL, pre + "gamma must be finite and > 0");
    if (width > GNX_RBF_MAX_WIDTH) return gnx_fail(ctx, GNX_EINVAL, pre + "window wider than GNX_RBF_MAX_WIDTH SNPs");
    if ((uint64_t)N * N * 8 > GNX_SVC_GRAM_BUDGET)
      return gnx_fail(ctx, GNX_EINVAL, pre + "one window's Gram and distances (2 N^2 words) exceed GNX_SVC_GRAM_BUDGET");
    return GNX_OK;
  }
  uint64_t gw = 0;
  if (kernel_kind == GNX_SVC_KERNEL_POLY) {
    if (!(poly->p > 0.0) || !std::isfinite(poly->p)) return gnx_fail(ctx, GNX_EINVAL, pre + "poly_p must be finite and > 0");
    if (!poly->run_value) return gnx_fail(ctx, GNX_EINVAL, pre + "run_value is NULL");
    if (width > SVC_POLY_MAX_WIDTH)
      return gnx_fail(ctx, GNX_EINVAL, pre + "window of " + std::to_string(width) + " SNPs: the polynomial kernel's run values (8 bytes each) "
                                         "must fit " + std::to_string(SVC_POLY_LDS_BUDGET >> 10) + " KiB of LDS: at most " +
                                         std::to_string(SVC_POLY_MAX_WIDTH) + " SNPs");
    if (poly->n < width + 1)
      return gnx_fail(ctx, GNX_EINVAL, pre + "run_value holds " + std::to_string(poly->n) + " values, a window of " + std::to_string(width) +
                                         " SNPs needs " + std::to_string(width + 1));
    for (int64_t L = 0; L <= width; ++L)
      if (!(poly->run_value[L] >= 0.0) || !std::isfinite(poly->run_value[L]))
        return gnx_fail(ctx, GNX_EINVAL, pre + "run_value[" + std::to_string(L) + "] is negative or not finite");
    // the largest kernel value: K(x, x) = run_value[width] / p for p >= 1 (L^p is superadditive); below 1 runs of one SNP add up to
    // at most width / p
    const double top = std::max(poly->run_value[width], poly->p < 1.0 ? (double)width : 0.0) / poly->p;
    gw = top < 1.8e19 ? (uint64_t)(long long)top : ~(uint64_t)0;
  } else {
    if (width > SVC_MAX_WIDTH) return gnx_fail(ctx, GNX_EINVAL, pre + "window wider than " + std::to_string(SVC_MAX_WIDTH) + " SNPs");
    // the largest kernel value is K(x, x) = g(width): it must be an exact float
    for (int32_t m : kernel_lengths(kernel_kind, (int)width)) gw += (uint64_t)(width - m + 1);
  }
  if (gw >= ((uint64_t)1 << 24))
    return gnx_fail(ctx, GNX_EINVAL, pre + "window of " + std::to_string(width) + " SNPs: kernel values reach " + std::to_string(gw) +
                                       " >= 2^24, not exact in float");
  if ((uint64_t)N * N * 4 > GNX_SVC_GRAM_BUDGET)
    return gnx_fail(ctx, GNX_EINVAL, pre + "one window's Gram (N^2 floats) exceeds GNX_SVC_GRAM_BUDGET");
  return GNX_OK;
}

int train_svc_check(gnx_ctx* ctx, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t cx, int32_t A, const gnx_svc_params* prm,
                    const SvcPoly* poly, const void* X, const void* y, const uint32_t* seeds, const void* o1, const void* o2, const void* o3,
                    const void* o4, const void* o5, const void* o6, const void* o7) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (!prm) return gnx_fail(ctx, GNX_EINVAL, "train_svc: params is NULL");
  const int32_t kernel_kind = prm->kernel_kind;
  if (!X || !y || !seeds || !o1 || !o2 || !o3 || !o4 || !o5 || !o6 || !o7) return gnx_fail(ctx, GNX_EINVAL, "train_svc: NULL array");
  if (A < 2 || A > 32) return gnx_fail(ctx, GNX_EINVAL, "A (ancestries) must be in [2, 32]");
  if (N < 2 || N > INT32_MAX || M <= 0 || C < M || cx < 0 || cx > C || ldx < C || C > INT32_MAX)
    return gnx_fail(ctx, GNX_EINVAL, "train_svc: bad N / C / M / ctx / ldx");
  if (poly && kernel_kind != GNX_SVC_KERNEL_POLY)
    return gnx_fail(ctx, GNX_EINVAL, "train_svc_poly: kernel_kind must be GNX_SVC_KERNEL_POLY (the other kinds: gnx_train_svc2)");
  if (kernel_kind == GNX_SVC_KERNEL_POLY && !poly)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, "train_svc: the polynomial string kernel (GNX_SVC_KERNEL_POLY) takes its exponent and run "
                                           "values through gnx_train_svc_poly");
  if (kernel_kind != GNX_SVC_KERNEL_SUBSTRINGS && kernel_kind != GNX_SVC_KERNEL_ALL_LENGTHS && kernel_kind != GNX_SVC_KERNEL_RBF && !poly)
    return gnx_fail(ctx, GNX_EINVAL, "train_svc: kernel_kind must be GNX_SVC_KERNEL_SUBSTRINGS, GNX_SVC_KERNEL_ALL_LENGTHS or GNX_SVC_KERNEL_RBF");
  if (!(prm->C > 0.0) || !std::isfinite(prm->C)) return gnx_fail(ctx, GNX_EINVAL, "train_svc: C must be finite and > 0");
  return svc_kernel_check(ctx, "train_svc", N, C, M, cx, kernel_kind, prm->gamma, poly);
}

int train_svc_labels(gnx_ctx* ctx, const int32_t* y, int64_t N, int W, int32_t A) {
  for (int64_t i = 0; i < N * W; ++i)
    if (y[i] < 0 || y[i] >= A) return gnx_fail(ctx, GNX_EINVAL, "train_svc: label outside [0, A)");
  std::vector<int64_t> cnt(A);
  for (int w = 0; w < W; ++w) {
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int64_t n = 0; n < N; ++n) cnt[y[n * W + w]]++;
    for (int c = 0; c < A; ++c)
      if (!cnt[c])
        return gnx_fail(ctx, GNX_EINVAL, "train_svc: window " + std::to_string(w) + " has no training row of class " + std::to_string(c) +
                                           " (the reference's fit fails there)");
  }
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_svc_fold_permutation(uint32_t seed, int32_t l, int32_t* perm) {
  if (l < 0 || (l > 0 && !perm)) return GNX_EINVAL;
  fold_permutation(seed, l, perm);
  return GNX_OK;
}

namespace {

int train_svc_dev_any(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t ctx_snps,
                      int32_t A, const gnx_svc_params* params, const SvcPoly* poly, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support,
                      int32_t* support, double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info) {
  if (!ctx) return GNX_EINVAL;
  int rc = train_svc_check(ctx, N, ldx, C, M, ctx_snps, A, params, poly, dX, dy, seeds, n_sv, n_support, support, dual_coef, intercept,
                           prob_a, prob_b);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  const int W = (int)(C / M);
  std::vector<int32_t> y((size_t)N * W);
  HIPCHK(ctx, hipMemcpyAsync(y.data(), dy, y.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = train_svc_labels(ctx, y.data(), N, W, A)) != GNX_OK) return rc;
  return train_svc_impl(ctx, dX, N, ldx, y.data(), C, M, ctx_snps, A, *params, poly, seeds, n_sv, n_support, support, dual_coef, intercept,
                        prob_a, prob_b, info);
}

int train_svc_host_any(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t ctx_snps,
                       int32_t A, const gnx_svc_params* params, const SvcPoly* poly, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support,
                       int32_t* support, double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info) {
  if (!ctx) return GNX_EINVAL;
  int rc = train_svc_check(ctx, N, ldx, C, M, ctx_snps, A, params, poly, X, y, seeds, n_sv, n_support, support, dual_coef, intercept,
                           prob_a, prob_b);
  if (rc != GNX_OK) return rc;
  if ((rc = train_svc_labels(ctx, y, N, (int)(C / M), A)) != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  gnx_dev_tmp xb;
  hipError_t e = xb.alloc((size_t)N * C + 64);
  if (e != hipSuccess) {
    xb.p = nullptr;
    return gnx_fail(ctx, GNX_ENOMEM, std::string("train_svc: hipMalloc: ") + hipGetErrorString(e));
  }
  HIPCHK(ctx, hipMemcpy2DAsync(xb.p, (size_t)C, X, (size_t)ldx, (size_t)C, (size_t)N, hipMemcpyHostToDevice, ctx->stream));
  return train_svc_impl(ctx, (const int8_t*)xb.p, N, C, y, C, M, ctx_snps, A, *params, poly, seeds, n_sv, n_support, support, dual_coef,
                        intercept, prob_a, prob_b, info);
}

}  // namespace

extern "C" int gnx_train_svc2_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                                  int64_t ctx_snps, int32_t A, const gnx_svc_params* params, const uint32_t* seeds, int32_t* n_sv,
                                  int32_t* n_support, int32_t* support, double* dual_coef, double* intercept, double* prob_a,
                                  double* prob_b, gnx_svc_train_info* info) {
  return train_svc_dev_any(ctx, dX, N, ldx, dy, C, M, ctx_snps, A, params, nullptr, seeds, n_sv, n_support, support, dual_coef, intercept,
                           prob_a, prob_b, info);
}

extern "C" int gnx_train_svc2(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M,
                              int64_t ctx_snps, int32_t A, const gnx_svc_params* params, const uint32_t* seeds, int32_t* n_sv,
                              int32_t* n_support, int32_t* support, double* dual_coef, double* intercept, double* prob_a, double* prob_b,
                              gnx_svc_train_info* info) {
  return train_svc_host_any(ctx, X, N, ldx, y, C, M, ctx_snps, A, params, nullptr, seeds, n_sv, n_support, support, dual_coef, intercept,
                            prob_a, prob_b, info);
}

// PolynomialStringKernelBase: params->kernel_kind = GNX_SVC_KERNEL_POLY, the exponent and the run values beside it
extern "C" int gnx_train_svc_poly_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                                      int64_t ctx_snps, int32_t A, const gnx_svc_params* params, double poly_p, const double* run_value,
                                      int64_t n_run_value, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support,
                                      double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info) {
  const SvcPoly poly{poly_p, run_value, n_run_value};
  return train_svc_dev_any(ctx, dX, N, ldx, dy, C, M, ctx_snps, A, params, &poly, seeds, n_sv, n_support, support, dual_coef, intercept,
                           prob_a, prob_b, info);
}

extern "C" int gnx_train_svc_poly(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M,
                                  int64_t ctx_snps, int32_t A, const gnx_svc_params* params, double poly_p, const double* run_value,
                                  int64_t n_run_value, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support, int32_t* support,
                                  double* dual_coef, double* intercept, double* prob_a, double* prob_b, gnx_svc_train_info* info) {
  const SvcPoly poly{poly_p, run_value, n_run_value};
  return train_svc_host_any(ctx, X, N, ldx, y, C, M, ctx_snps, A, params, &poly, seeds, n_sv, n_support, support, dual_coef, intercept,
                            prob_a, prob_b, info);
}

// the float Gram matrices of windows [w0, w1) as the trainers compute them (k_svc_pack + k_svc_gram / k_svc_gram_poly): host pointers
extern "C" int gnx_svc_gram(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t ctx_snps, int32_t kernel_kind,
                            double poly_p, const double* run_value, int64_t n_run_value, int64_t w0, int64_t w1, float* gram) {
  if (!ctx) return GNX_EINVAL;
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (!X || !gram) return gnx_fail(ctx, GNX_EINVAL, "svc_gram: NULL array");
  if (N < 1 || N > INT32_MAX || M <= 0 || C < M || ctx_snps < 0 || ctx_snps > C || ldx < C || C > INT32_MAX)
    return gnx_fail(ctx, GNX_EINVAL, "svc_gram: bad N / C / M / ctx / ldx");
  const int W = (int)(C / M);
  if (w0 < 0 || w1 <= w0 || w1 > W) return gnx_fail(ctx, GNX_EINVAL, "svc_gram: windows [w0, w1) must lie in [0, W) and hold at least one");
  if (kernel_kind != GNX_SVC_KERNEL_SUBSTRINGS && kernel_kind != GNX_SVC_KERNEL_ALL_LENGTHS && kernel_kind != GNX_SVC_KERNEL_POLY)
    return gnx_fail(ctx, GNX_EINVAL, "svc_gram: kernel_kind must be GNX_SVC_KERNEL_SUBSTRINGS, GNX_SVC_KERNEL_POLY or GNX_SVC_KERNEL_ALL_LENGTHS");
  const bool is_poly = kernel_kind == GNX_SVC_KERNEL_POLY;
  const SvcPoly poly{poly_p, run_value, n_run_value};
  int rc = svc_kernel_check(ctx, "svc_gram", N, C, M, ctx_snps, kernel_kind, 0.0, is_poly ? &poly : nullptr);
  if (rc != GNX_OK) return rc;
  const size_t gram_w = (size_t)N * N * 4;
  if ((uint64_t)(w1 - w0) * gram_w > GNX_SVC_GRAM_BUDGET)
    return gnx_fail(ctx, GNX_EINVAL, "svc_gram: the Gram matrices of the range exceed GNX_SVC_GRAM_BUDGET: ask for fewer windows");
  GNX_BIND_DEVICE(ctx);
  const int width_main = (int)(M + 2 * ctx_snps), width_last = width_main + (int)(C % M), nwm = (width_last + 31) / 32;
  const int wb = (int)std::min<int64_t>(w1 - w0, SVC_MAX_BATCH);
  const std::vector<uint32_t> g = is_poly ? std::vector<uint32_t>(width_last + 1, 0) : run_table(kernel_kind, width_last);
  const size_t bX = up256((size_t)N * C + 64), bPl = up256((size_t)wb * N * 2 * nwm * 4), bGram = up256((size_t)wb * gram_w);
  const size_t bG = up256((size_t)(width_last + 1) * 4), bRv = is_poly ? up256((size_t)(width_last + 1) * 8) : 0;
  gnx_dev_tmp blk;
  hipError_t e = blk.alloc(bX + bPl + bGram + bG + bRv);
  if (e != hipSuccess) {
    blk.p = nullptr;
    return gnx_fail(ctx, GNX_ENOMEM, std::string("svc_gram: hipMalloc: ") + hipGetErrorString(e));
  }
  char* q = (char*)blk.p;
  auto take = [&](size_t b) { char* r = q; q += b; return r; };
  int8_t* dX = (int8_t*)take(bX);
  uint32_t* dPl = (uint32_t*)take(bPl);
  float* dGram = (float*)take(bGram);
  uint32_t* dg = (uint32_t*)take(bG);
  double* dRv = is_poly ? (double*)take(bRv) : nullptr;
  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipMemcpy2DAsync(dX, (size_t)C, X, (size_t)ldx, (size_t)C, (size_t)N, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dg, g.data(), (size_t)(width_last + 1) * 4, hipMemcpyHostToDevice, s));
  if (is_poly) HIPCHK(ctx, hipMemcpyAsync(dRv, run_value, (size_t)(width_last + 1) * 8, hipMemcpyHostToDevice, s));
  const GramPass gp{N, nwm, W, width_main, width_last, dg, dRv, is_poly ? poly_p : 0.0};
  HIPCHK(ctx, gram_pass_prepare(gp));
  for (int64_t w = w0; w < w1; w += wb) {
    const int nb = (int)std::min<int64_t>(wb, w1 - w);
    HIPCHK(ctx, gram_pass(gp, dX, C, C, M, ctx_snps, (int)w, nb, dPl, dGram, s));
    HIPCHK(ctx, hipMemcpyAsync(gram + (size_t)(w - w0) * N * N, dGram, (size_t)nb * gram_w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return GNX_OK;
}

// the CovRSK entries: C = 1 (sklearn's default)
extern "C" int gnx_train_svc_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M,
                                 int64_t ctx_snps, int32_t A, int32_t kernel_kind, const uint32_t* seeds, int32_t* n_sv,
                                 int32_t* n_support, int32_t* support, double* dual_coef, double* intercept, double* prob_a,
                                 double* prob_b, gnx_svc_train_info* info) {
  if (ctx && kernel_kind == GNX_SVC_KERNEL_RBF) return gnx_fail(ctx, GNX_EINVAL, "train_svc: GNX_SVC_KERNEL_RBF needs gamma: use gnx_train_svc2");
  const gnx_svc_params prm{kernel_kind, 0, 1.0, 0.0};
  return gnx_train_svc2_dev(ctx, dX, N, ldx, dy, C, M, ctx_snps, A, &prm, seeds, n_sv, n_support, support, dual_coef, intercept, prob_a,
                            prob_b, info);
}

extern "C" int gnx_train_svc(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M,
                             int64_t ctx_snps, int32_t A, int32_t kernel_kind, const uint32_t* seeds, int32_t* n_sv, int32_t* n_support,
                             int32_t* support, double* dual_coef, double* intercept, double* prob_a, double* prob_b,
                             gnx_svc_train_info* info) {
  if (ctx && kernel_kind == GNX_SVC_KERNEL_RBF) return gnx_fail(ctx, GNX_EINVAL, "train_svc: GNX_SVC_KERNEL_RBF needs gamma: use gnx_train_svc2");
  const gnx_svc_params prm{kernel_kind, 0, 1.0, 0.0};
  return gnx_train_svc2(ctx, X, N, ldx, y, C, M, ctx_snps, A, &prm, seeds, n_sv, n_support, support, dual_coef, intercept, prob_a, prob_b,
                        info);
}
