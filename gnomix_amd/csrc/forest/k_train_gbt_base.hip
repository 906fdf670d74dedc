// forest/k_train_gbt_base.hip — training the boosted-tree BASE (XGBBase) on gfx950, all windows at once.
//
// Replaces Base.train of XGBBase (reference src/Base/base.py:104-127 -> src/Base/models.py:24-35: per window
// XGBClassifier(n_estimators=20, max_depth=4, learning_rate=0.1, reg_lambda=1, reg_alpha=0, missing=2).fit(Xw, yw)).  xgboost is a
// third-party fitter that is not part of the reference tree, so what is rebuilt is the ALGORITHM that call asks for, not xgboost's own
// floating-point trajectory (parity with xgboost itself is unpinned, as for k_train_gbt.hip).  Correctness is exact agreement with an
// independent CPU restatement (tests/gbt_base_exact.py).
//
// THE ALGORITHM (for every window w independently)
//   rows      n < N; features j < width_w = M + 2 ctx (+ C % M for the last window): feature j is column pad_src(w M + j) of X, the
//             window's reflect-padded slice (train.window_columns); label y[n, w].
//   codes     X holds 0, 1 and 2 = missing.  The trainer only ever COMPARES a code with 1 and with 2: any other value trains as 0
//             (it is never an index).  The host entry refuses such values; the _dev entry does not read X back.
//   objective A >= 3: multi:softprob, K = A trees per round, tree k of a round adds to class k; margins start at base_score.
//             A == 2: binary:logistic, K = 1 tree per round on the label y == 1; the margin starts at float(log(bs / (1 - bs))) (= 0).
//             Margins are float32 and take each round's leaf with one float32 addition.
//   gradients gnx_gbt_core.h's, shared with the smoother's trainer; det_exp is gnx_det_exp.h's fixed-order float64 exp.
//             multi:  m = max_c F_c (float32), e_c = det_exp(double(F_c - m)), s = sum e_c in class order, p_c = e_c / s,
//                     g = p_c - [y == c], h = max(2 p_c (1 - p_c), 1e-16)              (gbt_softprob_row)
//             binary: z = double(F), e = det_exp(-|z|), p = z >= 0 ? 1 / (1 + e) : e / (1 + e), g = p - [y == 1],
//                     h = max(p (1 - p), 1e-16)                                        (gbt_logistic_row)
//             both rounded to multiples of 2^-30: gi = llrint(g 2^30), hi = llrint(h 2^30).  EVERY sum below is an int64 of those, so
//             no result depends on scheduling, atomics order or tile order.
//   loss[r]   mean over the N W problems of -log(max(p_y, 1e-300)) before round r (r = n_rounds: after the last), float64
//             (binary: p_y = y == 1 ? p : 1 - p; a label outside [0, A) has p_y = 0 in the multi-class form).
//   node      (G, H) = its rows' sums.  For a feature, (G1, H1) and (Gm, Hm) are the sums over its rows with code 1 and code 2, the
//             code-0 sums are the node's minus both.  Candidates, in this order, left | right:
//               1: cond 0.5, missing right  {0} | {1, missing}       2: cond 0.5, missing left  {0, missing} | {1}
//               3: cond 1.5, missing right  {0, 1} | {missing}
//             gain = (GL^2 / (HL + lambda) + GR^2 / (HR + lambda)) - G^2 / (H + lambda) in float64 on the sums / 2^30, operations in
//             that order.  A candidate is valid if HL >= min_child_weight, HR >= min_child_weight and gain > max(gamma, 1e-6)
//             (gbt_split_gain, gbt_gain_floor).  The largest gain wins; ties go to the lowest feature, then the lowest candidate
//             (gbt_beats): a node without missing rows learns "default right".  No valid candidate, or depth max_depth reached: a
//             leaf, value float32(eta * (-(G / 2^30) / (H / 2^30 + lambda))) (gbt_leaf_value).
//
// THE STRUCTURE.  The hot loop is the per-level table of (G1, H1, Gm, Hm) for every (window, tree of the round, node, feature).  A row
// sits in exactly ONE node of a tree, so the dense form of that table — indicator planes times node-masked gradient columns on the
// int8 matrix cores — multiplies the visits by the node count (up to 16) and by the ~9 int8 limbs a 31-bit (g, h) pair splits into.
// Built instead: a block takes one (window, tree, node), a chunk of FBT_CHUNK features (one per thread) and a slice of FBT_SLICE
// rows; it first compacts the slice's rows OF THAT NODE, with their (g, h), into LDS (one pass over the position bytes), then every
// thread walks that list: the row index and (g, h) are wave-uniform LDS broadcasts, the code is one coalesced byte load, and the
// sums are four predicated int64 additions in REGISTERS — no atomics per matrix entry, no runtime-indexed arrays, no scratch.  One
// int64 global atomic per (feature, sum) and block folds the row slices together (exact: integers).  The overlap of the windows
// (a SNP belongs to up to ceil((M + 2 ctx) / M) windows) is left to the L2: X is read in place, never expanded per window.
// All W windows train together: one launch sequence per round (gradients; per level: table, split search, row partition; leaves;
// margins), W never appears as a host loop.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../gnx_internal.h"
#include "../gnx_window.h"
#include "gnx_gbt_core.h"

namespace {

constexpr int FBT_CHUNK = 256;         // features of one histogram block (one per thread)
constexpr int FBT_SLICE = 2048;        // rows of one histogram block: (index, g, h) = 20 bytes each, 40 KB of LDS

struct FGeom {
  int64_t N, ldx, C, M, ctx;
  int32_t W, rem, A, K, maxw, R;  // K trees per round, R rounds
};

__device__ __forceinline__ int fbt_width(int w, const FGeom& G) { return (int)(G.M + 2 * G.ctx) + (w == G.W - 1 ? G.rem : 0); }

// node tables of tree (w, round r, k): [((w R + r) K + k)][GBT_MAXN]
__device__ __forceinline__ size_t fbt_tab(int w, int r, int k, const FGeom& G) { return (((size_t)w * G.R + r) * G.K + k) * GBT_MAXN; }

// gradients of one round: block = 256 rows of one window.  Root sums per tree (int64, exact), the block's loss in a fixed order.
// fit == 0: only the loss (the pass after the last round).
template <int AMAX>
__global__ __launch_bounds__(256) void k_fbt_grad(const float* Fm, const int32_t* y, long long* gq, long long* hq, uint8_t* pos, long long* tG,
                                                   long long* tH, int32_t* tS, double* loss_part, int r, int fit, int nb, FGeom G) {
  __shared__ long long sg[AMAX], sh[AMAX];
  __shared__ double sl[256];
  const int w = blockIdx.x / nb, b = blockIdx.x - w * nb;
  const int A = G.A, K = G.K;
  if (threadIdx.x < AMAX) { sg[threadIdx.x] = 0; sh[threadIdx.x] = 0; }
  __syncthreads();
  const int64_t n = (int64_t)b * 256 + threadIdx.x;
  double l = 0.0;
  if (n < G.N) {
    const float* f = Fm + ((size_t)w * G.N + n) * K;
    const int yi = y[n * G.W + w];
    auto emit = [&](int c, long long gi, long long hi) {  // tree c of the round
      if (!fit) return;
      const size_t o = ((size_t)w * K + c) * G.N + n;
      gq[o] = gi; hq[o] = hi; pos[o] = 0;
      atomicAdd(reinterpret_cast<unsigned long long*>(&sg[c]), (unsigned long long)gi);
      atomicAdd(reinterpret_cast<unsigned long long*>(&sh[c]), (unsigned long long)hi);
    };
    const double py = K == 1 ? gbt_logistic_row(f[0], yi, emit) : gbt_softprob_row<AMAX>(f, A, yi, emit);
    l = -log(py > 1e-300 ? py : 1e-300);
  }
  sl[threadIdx.x] = l;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // a fixed tree: the same bits whatever the schedule
    if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_part[blockIdx.x] = sl[0];
  if (fit && (int)threadIdx.x < K) {
    const size_t o = fbt_tab(w, r, threadIdx.x, G);
    atomicAdd(reinterpret_cast<unsigned long long*>(&tG[o]), (unsigned long long)sg[threadIdx.x]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&tH[o]), (unsigned long long)sh[threadIdx.x]);
    tS[o] = 1;  // (every block writes the same value)
  }
}

// the blocks' losses, summed by one block in a fixed order -> mean over the N W problems
__global__ __launch_bounds__(256) void k_fbt_loss(const double* part, int64_t n_part, double* loss, double inv_count) {
  __shared__ double sl[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += 256) a += part[i];
  sl[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = sl[0] * inv_count;
}

// the level's table: hist[((w K + k) nl + node of level) maxw + j][4] = (G1, H1, Gm, Hm).
// grid (w K + k, feature chunk x row slice, node of level); see the header for the structure.
__global__ __launch_bounds__(FBT_CHUNK) void k_fbt_hist(const int8_t* __restrict__ X, const long long* __restrict__ gq, const long long* __restrict__ hq,
                                                         const uint8_t* __restrict__ pos, const int32_t* __restrict__ tS, long long* hist, int r,
                                                         int d, int n_chunks, int n_slices, FGeom G) {
  __shared__ int32_t ln[FBT_SLICE];
  __shared__ long long lg[FBT_SLICE], lh[FBT_SLICE];
  __shared__ int cnt;
  const int nl = 1 << d, node = nl - 1 + (int)blockIdx.z;
  const int wk = blockIdx.x, w = wk / G.K, k = wk - w * G.K;
  if (tS[fbt_tab(w, r, k, G) + node] != 1) return;  // not an open node (uniform over the block)
  const int chunk = blockIdx.y % n_chunks, slice = blockIdx.y / n_chunks;
  const int width = fbt_width(w, G);
  if (chunk * FBT_CHUNK >= width) return;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)slice * FBT_SLICE, r1 = min(G.N, r0 + FBT_SLICE);
  const size_t row0 = (size_t)wk * G.N;
  for (int64_t n = r0 + threadIdx.x; n < r1; n += FBT_CHUNK)
    if (pos[row0 + n] == node) {
      const int slot = atomicAdd(&cnt, 1);  // slot < r1 - r0 <= FBT_SLICE; any order: the sums are integers
      ln[slot] = (int32_t)n; lg[slot] = gq[row0 + n]; lh[slot] = hq[row0 + n];
    }
  __syncthreads();
  const int rows = cnt;
  const int j = chunk * FBT_CHUNK + threadIdx.x;
  if (j >= width || (rows == 0 && n_slices > 1)) return;  // (a single slice stores: an empty node stores zeros)
  const int8_t* xc = X + gnx_pad_src((int64_t)w * G.M + j, G.C, G.ctx);
  long long G1 = 0, H1 = 0, Gm = 0, Hm = 0;
#pragma unroll 4
  for (int i = 0; i < rows; ++i) {
    const int x = xc[(int64_t)ln[i] * G.ldx];
    const long long g = lg[i], h = lh[i];
    G1 += x == 1 ? g : 0; H1 += x == 1 ? h : 0;
    Gm += x == 2 ? g : 0; Hm += x == 2 ? h : 0;
  }
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(hist + (((size_t)wk * nl + blockIdx.z) * G.maxw + j) * 4);
  if (n_slices == 1) {
    dst[0] = (unsigned long long)G1; dst[1] = (unsigned long long)H1; dst[2] = (unsigned long long)Gm; dst[3] = (unsigned long long)Hm;
  } else {  // (the table is zeroed before the launch)
    atomicAdd(dst + 0, (unsigned long long)G1); atomicAdd(dst + 1, (unsigned long long)H1);
    atomicAdd(dst + 2, (unsigned long long)Gm); atomicAdd(dst + 3, (unsigned long long)Hm);
  }
}

// best split of every open node of the level: grid (w K + k, node of level); a thread per feature, three candidates each
__global__ __launch_bounds__(256) void k_fbt_split(const long long* __restrict__ hist, GbtTables t, int r, int d, double lambda, double gamma,
                                                    double mcw, FGeom G) {
  const int nl = 1 << d, kk = blockIdx.y, node = nl - 1 + kk;
  const int wk = blockIdx.x, w = wk / G.K, k = wk - w * G.K;
  const size_t o = fbt_tab(w, r, k, G);
  if (t.S[o + node] != 1) return;
  const int width = fbt_width(w, G);
  const long long Gn = t.G[o + node], Hn = t.H[o + node];
  const double root_term = gbt_root_term(Gn, Hn, lambda), floor_ = gbt_gain_floor(gamma);
  // the running best as scalars (see gbt_block_best); a candidate exists iff bf >= 0
  double bg = 0.0;
  int bf = -1, bc = 0;
  long long bGL = 0, bHL = 0;
  const long long* hrow = hist + ((size_t)wk * nl + kk) * G.maxw * 4;
  for (int j = threadIdx.x; j < width; j += 256) {
    const long long G1 = hrow[(size_t)j * 4], H1 = hrow[(size_t)j * 4 + 1], Gm = hrow[(size_t)j * 4 + 2], Hm = hrow[(size_t)j * 4 + 3];
#pragma unroll
    for (int c = 1; c <= 3; ++c) {
      const long long GL = c == 1 ? Gn - G1 - Gm : (c == 2 ? Gn - G1 : Gn - Gm);
      const long long HL = c == 1 ? Hn - H1 - Hm : (c == 2 ? Hn - H1 : Hn - Hm);
      double gain;
      if (!gbt_split_gain(GL, HL, Gn, Hn, root_term, lambda, mcw, &gain) || !(gain > floor_)) continue;
      if (bf < 0 || gain > bg) { bg = gain; bf = j; bc = c; bGL = GL; bHL = HL; }  // (j and c ascend: the first of equals stays)
    }
  }
  gbt_block_best(bg, bf, bc, bGL, bHL);
  if (threadIdx.x == 0) gbt_commit_split(t, o, node, bf >= 0, bf, bc, bGL, bHL);
}

// rows of the nodes split at level d move to their children: grid (blocks of rows, w K + k)
__global__ __launch_bounds__(256) void k_fbt_partition(const int8_t* __restrict__ X, uint8_t* pos, const int32_t* __restrict__ tS,
                                                        const int32_t* __restrict__ tF, const int32_t* __restrict__ tC, int r, int d, int nb, FGeom G) {
  const int wk = blockIdx.x / nb, b = blockIdx.x - wk * nb;
  const int w = wk / G.K, k = wk - w * G.K;
  const int64_t n = (int64_t)b * 256 + threadIdx.x;
  if (n >= G.N) return;
  const size_t o = fbt_tab(w, r, k, G), i = (size_t)wk * G.N + n;
  const int node = pos[i];
  if (node < (1 << d) - 1 || tS[o + node] != 2) return;
  const int x = X[n * G.ldx + gnx_pad_src((int64_t)w * G.M + tF[o + node], G.C, G.ctx)];
  const int c = tC[o + node];
  // candidate 1: {0} | {1, m};  2: {0, m} | {1};  3: {0, 1} | {m}   (a code that is neither 1 nor 2 is a 0)
  const bool left = c == 1 ? (x != 1 && x != 2) : (c == 2 ? x != 1 : x != 2);
  pos[i] = (uint8_t)(left ? 2 * node + 1 : 2 * node + 2);
}

// leaves of the round: every node still open becomes one
__global__ __launch_bounds__(256) void k_fbt_close(GbtTables t, int r, int64_t total, double eta, double lambda, FGeom G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t wk = e / GBT_MAXN;
  const int node = (int)(e - wk * GBT_MAXN), w = (int)(wk / G.K), k = (int)(wk - (int64_t)w * G.K);
  gbt_close_node(t, fbt_tab(w, r, k, G) + node, eta, lambda);
}

__global__ __launch_bounds__(256) void k_fbt_margin(float* Fm, const uint8_t* pos, const float* tV, int r, int64_t total, FGeom G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // e = (w N + n) K + k
  if (e >= total) return;
  const int k = (int)(e % G.K);
  const int64_t wn = e / G.K, w = wn / G.N, n = wn - w * G.N;
  Fm[e] += tV[fbt_tab((int)w, r, k, G) + pos[((size_t)w * G.K + k) * G.N + n]];
}

// per-phase wall times of the last run (gnx_train_gbt_base_phases): gradients + loss, table, split search, partition, leaves + margins
bool g_phases_on = false;
double g_phase_ms[5] = {0, 0, 0, 0, 0};

}  // namespace

// dX (N, ldx) int8 and dy (N, W) int32 on the device.  Host outputs as in gnx_train_gbt_base (include/gnomix_hip.h).
static hipError_t gnx_train_gbt_base_run(const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t ctx, int32_t A,
                                  const gnx_gbt_params& P, int32_t* win_tree0, int32_t* tree_off, int32_t* left, int32_t* right, int32_t* feat,
                                  float* cond, uint8_t* default_left, int32_t* tree_class, int64_t* n_nodes_out, double* loss_out, hipStream_t s) {
  FGeom G;
  G.N = N; G.ldx = ldx; G.C = C; G.M = M; G.ctx = ctx;
  G.W = (int32_t)(C / M); G.rem = (int32_t)(C - M * (C / M)); G.A = A; G.K = A == 2 ? 1 : A; G.maxw = (int32_t)(M + 2 * ctx) + G.rem;
  G.R = P.n_rounds;
  const int D = P.max_depth, W = G.W, K = G.K, R = G.R;
  const int64_t WK = (int64_t)W * K, rows = WK * N;
  const size_t tab_n = (size_t)WK * R * GBT_MAXN;
  const int nb = (int)((N + 255) / 256);
  const int n_chunks = (G.maxw + FBT_CHUNK - 1) / FBT_CHUNK, n_slices = (int)((N + FBT_SLICE - 1) / FBT_SLICE);
  const size_t hist_n = (size_t)WK * ((size_t)1 << (D - 1)) * G.maxw * 4;
  gnx_dev_tmp bFm, bG, bH, bPos, bTab, bHist, bPart, bLoss;
  GNX_HIPRET(bFm.alloc((size_t)rows * 4));
  GNX_HIPRET(bG.alloc((size_t)rows * 8));
  GNX_HIPRET(bH.alloc((size_t)rows * 8));
  GNX_HIPRET(bPos.alloc((size_t)rows));
  GbtTables t;
  GNX_HIPRET(gbt_tables_alloc(bTab, t, tab_n, s));
  GNX_HIPRET(bHist.alloc(hist_n * 8));
  GNX_HIPRET(bPart.alloc((size_t)W * nb * 8));
  GNX_HIPRET(bLoss.alloc((size_t)(R + 1) * 8));
  const float m0 = K == 1 ? (float)std::log(P.base_score / (1.0 - P.base_score)) : (float)P.base_score;
  hipLaunchKernelGGL(k_gbt_fill,dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, bFm.as<float>(), m0, rows);
  GNX_HIPRET(hipGetLastError());

  const bool prof = g_phases_on;
  double ms[5] = {0, 0, 0, 0, 0};
  auto t_prev = std::chrono::steady_clock::now();
  hipError_t perr = hipSuccess;
  auto phase = [&](int which) {  // (profiling only: a synchronisation per phase)
    if (!prof) return;
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess && perr == hipSuccess) perr = e;
    const auto t = std::chrono::steady_clock::now();
    if (which >= 0) ms[which] += std::chrono::duration<double, std::milli>(t - t_prev).count();
    t_prev = t;
  };
  auto grad = [&](int r, int fit) {
    const int rr = r < R ? r : R - 1;
#define FBT_GRAD(AM) hipLaunchKernelGGL(k_fbt_grad<AM>, dim3((unsigned)((int64_t)W * nb)), dim3(256), 0, s, bFm.as<float>(), dy, bG.as<long long>(), \
                                        bH.as<long long>(), bPos.as<uint8_t>(), t.G, t.H, t.S, bPart.as<double>(), rr, fit, nb, G)
    if (A <= 8) FBT_GRAD(8);
    else if (A <= 16) FBT_GRAD(16);
    else FBT_GRAD(32);
#undef FBT_GRAD
    hipLaunchKernelGGL(k_fbt_loss, dim3(1), dim3(256), 0, s, bPart.as<double>(), (int64_t)W * nb, bLoss.as<double>() + r, 1.0 / ((double)N * (double)W));
  };
  phase(-1);
  for (int r = 0; r < R; ++r) {
    grad(r, 1);
    GNX_HIPRET(hipGetLastError());
    phase(0);
    for (int d = 0; d < D; ++d) {
      const int nl = 1 << d;
      if (n_slices > 1) GNX_HIPRET(hipMemsetAsync(bHist.p, 0, (size_t)WK * nl * G.maxw * 32, s));
      hipLaunchKernelGGL(k_fbt_hist, dim3((unsigned)WK, (unsigned)(n_chunks * n_slices), (unsigned)nl), dim3(FBT_CHUNK), 0, s, dX, bG.as<long long>(),
                         bH.as<long long>(), bPos.as<uint8_t>(), t.S, bHist.as<long long>(), r, d, n_chunks, n_slices, G);
      phase(1);
      hipLaunchKernelGGL(k_fbt_split, dim3((unsigned)WK, (unsigned)nl), dim3(256), 0, s, bHist.as<long long>(), t, r, d, P.lambda, P.gamma,
                         P.min_child_weight, G);
      phase(2);
      hipLaunchKernelGGL(k_fbt_partition, dim3((unsigned)(WK * nb)), dim3(256), 0, s, dX, bPos.as<uint8_t>(), t.S, t.F, t.C, r, d, nb, G);
      phase(3);
    }
    hipLaunchKernelGGL(k_fbt_close, dim3((unsigned)((WK * GBT_MAXN + 255) / 256)), dim3(256), 0, s, t, r, WK * GBT_MAXN, P.eta, P.lambda, G);
    hipLaunchKernelGGL(k_fbt_margin, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, bFm.as<float>(), bPos.as<uint8_t>(), t.V, r, rows, G);
    GNX_HIPRET(hipGetLastError());
    phase(4);
  }
  grad(R, 0);
  GNX_HIPRET(hipGetLastError());
  phase(0);
  GNX_HIPRET(perr);

  // ---- trees back to the host: window-major, round-major, nodes in heap order ----
  GbtHostTables h;
  std::vector<double> hL((size_t)R + 1);
  GNX_HIPRET(h.fetch(t, tab_n, s));
  GNX_HIPRET(hipMemcpyAsync(hL.data(), bLoss.p, hL.size() * 8, hipMemcpyDeviceToHost, s));
  GNX_HIPRET(hipStreamSynchronize(s));
  const int64_t T = WK * R;
  *n_nodes_out = gbt_compact_trees(
      h.S, T, tree_off, left, right,
      [&](int64_t q, size_t i) {  // candidate 1: 0.5, missing right; 2: 0.5, missing left; 3: 1.5, missing right
        feat[q] = h.F[i]; cond[q] = h.B[i] == 3 ? 1.5f : 0.5f; default_left[q] = h.B[i] == 2 ? 1 : 0;
      },
      [&](int64_t q, size_t i) { feat[q] = 0; cond[q] = h.V[i]; default_left[q] = 0; });
  for (int64_t tr = 0; tr < T; ++tr) tree_class[tr] = (int32_t)(tr % K);
  for (int w = 0; w <= W; ++w) win_tree0[w] = w * R * K;
  if (loss_out)
    for (int r = 0; r <= R; ++r) loss_out[r] = hL[(size_t)r];
  if (prof) std::memcpy(g_phase_ms, ms, sizeof(ms));
  return hipSuccess;
}

// ---- training the boosted-tree base (XGBBase) --------------------------------------------------------------------
namespace {
int gbt_base_check(gnx_ctx* ctx, const void* X, const int32_t* y, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t cx, int32_t A,
                          const gnx_gbt_params* P, const void* o1, const void* o2, const void* o3, const void* o4, const void* o5, const void* o6,
                          const void* o7, const void* o8, const void* o9) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (N <= 0 || !X || !y || !P || !o1 || !o2 || !o3 || !o4 || !o5 || !o6 || !o7 || !o8 || !o9)
    return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: bad X / y / params / outputs (N must be positive)");
  if (A < 2 || A > 32) return gnx_fail(ctx, GNX_EINVAL, "A (ancestries) must be in [2, 32]");
  if (M <= 0 || C < M || cx < 0 || cx > C || ldx < C) return gnx_fail(ctx, GNX_EINVAL, "bad C / M / ctx / ldx");
  if (C % M == 0) return gnx_fail(ctx, GNX_EINVAL, "C % M == 0: the reference's window slicing (base.py:158) requires a remainder");
  if (P->n_rounds < 1 || P->n_rounds > 100000 || P->max_depth < 1 || P->max_depth > 5)
    return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: n_rounds >= 1, 1 <= max_depth <= 5");
  if (!(P->eta > 0.0) || !(P->lambda >= 0.0) || !(P->gamma >= 0.0) || !(P->min_child_weight >= 0.0))
    return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: eta > 0, lambda / gamma / min_child_weight >= 0");
  if (A == 2 && !(P->base_score > 0.0 && P->base_score < 1.0)) return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: binary:logistic needs 0 < base_score < 1");
  // grid and index limits: rows in int32, (window, tree, row block) and every tree's 63 node slots in one grid dimension
  const int64_t W = C / M, K = A == 2 ? 1 : A, width = M + 2 * cx + C % M;
  if (N >= ((int64_t)1 << 31) || width >= ((int64_t)1 << 24) || W * K * ((N + 255) / 256) >= ((int64_t)1 << 31) ||
      W * K * P->n_rounds * 63 >= ((int64_t)1 << 31) || ((width + 255) / 256) * ((N + 2047) / 2048) > 65535)
    return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: problem too large for one launch sequence");
  return GNX_OK;
}
}  // namespace

extern "C" {

int gnx_train_gbt_base_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx, int32_t A,
                           const gnx_gbt_params* P, int32_t* win_tree0, int32_t* tree_off, int32_t* left, int32_t* right, int32_t* feat,
                           float* cond, uint8_t* default_left, int32_t* tree_class, int64_t* n_nodes, double* loss) {
  if (!ctx) return GNX_EINVAL;
  int rc = gbt_base_check(ctx, dX, dy, N, ldx, C, M, cx, A, P, win_tree0, tree_off, left, right, feat, cond, default_left, tree_class, n_nodes);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  HIPCHK(ctx, gnx_train_gbt_base_run(dX, N, ldx, dy, C, M, cx, A, *P, win_tree0, tree_off, left, right, feat, cond, default_left, tree_class,
                                     n_nodes, loss, ctx->stream));
  return GNX_OK;
}

int gnx_train_gbt_base(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t cx, int32_t A,
                       const gnx_gbt_params* P, int32_t* win_tree0, int32_t* tree_off, int32_t* left, int32_t* right, int32_t* feat, float* cond,
                       uint8_t* default_left, int32_t* tree_class, int64_t* n_nodes, double* loss) {
  if (!ctx) return GNX_EINVAL;
  int rc = gbt_base_check(ctx, X, y, N, ldx, C, M, cx, A, P, win_tree0, tree_off, left, right, feat, cond, default_left, tree_class, n_nodes);
  if (rc != GNX_OK) return rc;
  const int64_t W = C / M;
  for (int64_t i = 0; i < N * W; ++i)
    if (y[i] < 0 || y[i] >= A) return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: label outside [0, A)");
  for (int64_t n = 0; n < N; ++n)
    for (int64_t j = 0; j < C; ++j)
      if ((uint8_t)X[n * ldx + j] > 2) return gnx_fail(ctx, GNX_EINVAL, "train_gbt_base: X holds a code outside {0, 1, 2}");
  GNX_BIND_DEVICE(ctx);
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_x, (size_t)N * ldx + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, (size_t)N * W * 4)) != GNX_OK) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_x.p, X, (size_t)(N - 1) * ldx + C, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, y, (size_t)N * W * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, gnx_train_gbt_base_run((const int8_t*)ctx->ws_x.p, N, ldx, (const int32_t*)ctx->ws_lab.p, C, M, cx, A, *P, win_tree0, tree_off, left,
                                     right, feat, cond, default_left, tree_class, n_nodes, loss, ctx->stream));
  return GNX_OK;
}

int gnx_train_gbt_base_phases(int32_t enable, double* ms) {
  if (enable >= 0) g_phases_on = enable != 0;
  if (ms) std::memcpy(ms, g_phase_ms, sizeof(g_phase_ms));
  return GNX_OK;
}

}  // extern "C"
