// forest/gnx_gbt_core.h — what the two boosted-tree trainers (k_train_gbt.hip: the tree smoother; forest/k_train_gbt_base.hip: the
// XGBBase windows) share: the ONE statement of the objective, the gain, the tie rule, the split commit, the leaf and the tree layout.
//
// Both are held bit-exact to restatements on the CPU (the oracle's gnxo_train_gbt, tests/gbt_base_exact.py) by the same arithmetic:
// gradients rounded to multiples of 2^-30 and summed as int64 (no sum depends on scheduling), gains in float64 on those sums / 2^30
// with the operations in one order, probabilities through det_exp.  How each trainer finds its candidates and lays out its rows
// stays in its own file.  Everything here has internal linkage: no symbol is exported.
#pragma once
#include <vector>

#include "../gnx_internal.h"
#include "gnx_det_exp.h"

namespace {

constexpr double GBT_FIX = 1073741824.0;  // 2^30: one unit of a fixed-point gradient or hessian
constexpr int GBT_MAXN = 63;              // heap positions of a tree of depth <= 5

// ---- node tables: [tree][GBT_MAXN] x {G, H (int64 sums), F (feature), B (the smoother's bin or threshold bits) = C (the base's
// candidate), S (state: 0 absent, 1 open, 2 split, 3 leaf), V (leaf value)}.  One allocation of bytes(tab_n), zeroed, carved in six. ----
struct GbtTables {
  long long *G, *H;
  int32_t* F;
  union { int32_t* B; int32_t* C; };
  int32_t* S;
  float* V;
  static size_t bytes(size_t tab_n) { return tab_n * (8 + 8 + 4 + 4 + 4 + 4); }
  void carve(void* base, size_t tab_n) {
    G = reinterpret_cast<long long*>(base);
    H = G + tab_n;
    F = reinterpret_cast<int32_t*>(H + tab_n);
    B = F + tab_n;
    S = B + tab_n;
    V = reinterpret_cast<float*>(S + tab_n);
  }
  GbtTables at(size_t o) const { return GbtTables{G + o, H + o, F + o, {B + o}, S + o, V + o}; }  // the tables from slot o on
};

inline hipError_t gbt_tables_alloc(gnx_dev_tmp& buf, GbtTables& t, size_t tab_n, hipStream_t s) {
  GNX_HIPRET(buf.alloc(GbtTables::bytes(tab_n)));
  t.carve(buf.p, tab_n);
  return hipMemsetAsync(buf.p, 0, GbtTables::bytes(tab_n), s);
}

// ---- the objective ----
// multi:softprob pair of one row with margins f[0 .. A): m = max_c f_c (float32), e_c = det_exp(double(f_c - m)), s = sum e_c in class
// order, p_c = e_c / s, g = p_c - [y == c], h = max(2 p_c (1 - p_c), 1e-16); emit(c, llrint(g 2^30), llrint(h 2^30)) per class.
// Returns p_y (0 for a label outside [0, A)).  AMAX >= A bounds the unrolled loops, so e[] stays in registers.
template <int AMAX, class Emit>
__device__ __forceinline__ double gbt_softprob_row(const float* f, int A, int yi, Emit emit) {
  float m = f[0];
  for (int c = 1; c < A; ++c) m = f[c] > m ? f[c] : m;
  double e[AMAX], sum = 0.0;
#pragma unroll
  for (int c = 0; c < AMAX; ++c)
    if (c < A) { e[c] = det_exp((double)(f[c] - m)); sum += e[c]; }
  double py = 0.0;
#pragma unroll
  for (int c = 0; c < AMAX; ++c)
    if (c < A) {
      const double p = e[c] / sum;
      const double g = p - (yi == c ? 1.0 : 0.0);
      double h = 2.0 * p * (1.0 - p);
      if (h < 1e-16) h = 1e-16;
      emit(c, llrint(g * GBT_FIX), llrint(h * GBT_FIX));
      if (yi == c) py = p;
    }
  return py;
}

// binary:logistic pair of one row with margin f0, one tree on the label y == 1: z = double(f0), e = det_exp(-|z|),
// p = z >= 0 ? 1 / (1 + e) : e / (1 + e), g = p - [y == 1], h = max(p (1 - p), 1e-16); emit(0, ...).  Returns p_y = y == 1 ? p : 1 - p.
template <class Emit>
__device__ __forceinline__ double gbt_logistic_row(float f0, int yi, Emit emit) {
  const double z = (double)f0;
  const double e = det_exp(z >= 0.0 ? -z : z);
  const double p = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
  const double g = p - (yi == 1 ? 1.0 : 0.0);
  double h = p * (1.0 - p);
  if (h < 1e-16) h = 1e-16;
  emit(0, llrint(g * GBT_FIX), llrint(h * GBT_FIX));
  return yi == 1 ? p : 1.0 - p;
}

// ---- the gain of a candidate ----
// the node's own term G^2 / (H + lambda), and the floor a gain has to exceed: max(gamma, 1e-6)
__device__ __forceinline__ double gbt_root_term(long long Gn, long long Hn, double lambda) {
  const double Gd = (double)Gn / GBT_FIX, Hd = (double)Hn / GBT_FIX;
  return Gd * Gd / (Hd + lambda);
}
__device__ __forceinline__ double gbt_gain_floor(double gamma) { return gamma > 1e-6 ? gamma : 1e-6; }

// (GL, HL) left | (Gn - GL, Hn - HL) right.  false: a child lighter than min_child_weight.  Else
// gain = (GL^2 / (HL + lambda) + GR^2 / (HR + lambda)) - root_term, float64, in that order; the caller holds it against the floor.
__device__ __forceinline__ bool gbt_split_gain(long long GL, long long HL, long long Gn, long long Hn, double root_term, double lambda, double mcw,
                                               double* gain) {
  const double gl = (double)GL / GBT_FIX, hl = (double)HL / GBT_FIX;
  const double gr = (double)(Gn - GL) / GBT_FIX, hr = (double)(Hn - HL) / GBT_FIX;
  if (hl < mcw || hr < mcw) return false;
  *gain = (gl * gl / (hl + lambda) + gr * gr / (hr + lambda)) - root_term;
  return true;
}

// ---- the tie rule and the block's best candidate ----
// larger gain, then lower feature, then lower bin (smoother) or candidate (base)
__device__ __forceinline__ bool gbt_beats(double g1, int f1, int j1, double g2, int f2, int j2) {
  return g1 > g2 || (g1 == g2 && (f1 < f2 || (f1 == f2 && j1 < j2)));
}

// The best of a 256-thread block's running bests (gain, f, j, GL, HL; a thread has a candidate iff f >= 0): 64-lane shuffle reduction,
// then the four waves through LDS.  The winner ends in thread 0's arguments (f stays < 0: no thread had one); every thread of the
// block must call.  The five values travel as SCALARS, and a winner is picked by index, never as a struct: hipcc 7.2 mixed the
// fields of two `Best` values in the select it built for `b = t`, here and in the pick kernels.
__device__ __forceinline__ void gbt_block_best(double& bg, int& bf, int& bj, long long& bGL, long long& bHL) {
  for (int o = 32; o > 0; o >>= 1) {
    const double tg = __shfl_down(bg, o);
    const int tf = __shfl_down(bf, o), tj = __shfl_down(bj, o);
    const long long tGL = __shfl_down(bGL, o), tHL = __shfl_down(bHL, o);
    if (tf >= 0 && (bf < 0 || gbt_beats(tg, tf, tj, bg, bf, bj))) { bg = tg; bf = tf; bj = tj; bGL = tGL; bHL = tHL; }
  }
  __shared__ double wg[4];
  __shared__ int wf[4], wj[4];
  __shared__ long long wGL[4], wHL[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { wg[wave] = bg; wf[wave] = bf; wj[wave] = bj; wGL[wave] = bGL; wHL[wave] = bHL; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int bw = -1;
    for (int w = 0; w < 4; ++w)
      if (wf[w] >= 0 && (bw < 0 || gbt_beats(wg[w], wf[w], wj[w], wg[bw], wf[bw], wj[bw]))) bw = w;
    if (bw > 0) { bg = wg[bw]; bf = wf[bw]; bj = wj[bw]; bGL = wGL[bw]; bHL = wHL[bw]; }  // (wave 0's best is this thread's own)
  }
}

// ---- committing a node's search, closing a round ----
// found: the node (heap position `node` of the tree whose tables start at slot o) splits on feature f with b, its children open with
// (GL, HL) and the rest; else it is a leaf
__device__ __forceinline__ void gbt_commit_split(const GbtTables& t, size_t o, int node, bool found, int f, int b, long long GL, long long HL) {
  if (!found) { t.S[o + node] = 3; return; }
  const long long Gn = t.G[o + node], Hn = t.H[o + node];
  t.S[o + node] = 2; t.F[o + node] = f; t.B[o + node] = b;
  const int l = 2 * node + 1, r = 2 * node + 2;
  t.S[o + l] = 1; t.S[o + r] = 1;
  t.G[o + l] = GL; t.H[o + l] = HL; t.G[o + r] = Gn - GL; t.H[o + r] = Hn - HL;
}

__device__ __forceinline__ float gbt_leaf_value(long long G, long long H, double eta, double lambda) {
  const double Gd = (double)G / GBT_FIX, Hd = (double)H / GBT_FIX;
  return (float)(eta * (-Gd / (Hd + lambda)));
}

// the end of a round for table slot i: a node still open becomes a leaf, every leaf gets its value
__device__ __forceinline__ void gbt_close_node(const GbtTables& t, size_t i, double eta, double lambda) {
  if (t.S[i] == 1) t.S[i] = 3;
  if (t.S[i] == 3) t.V[i] = gbt_leaf_value(t.G[i], t.H[i], eta, lambda);
}

__global__ __launch_bounds__(256) void k_gbt_fill(float* p, float v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- trees back to the host ----
struct GbtHostTables {
  std::vector<int32_t> F, B, S;
  std::vector<float> V;
  // enqueues the copies; the caller synchronises the stream (after whatever else it copies back)
  hipError_t fetch(const GbtTables& t, size_t tab_n, hipStream_t s) {
    F.resize(tab_n); B.resize(tab_n); S.resize(tab_n); V.resize(tab_n);
    GNX_HIPRET(hipMemcpyAsync(F.data(), t.F, tab_n * 4, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(B.data(), t.B, tab_n * 4, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(S.data(), t.S, tab_n * 4, hipMemcpyDeviceToHost, s));
    return hipMemcpyAsync(V.data(), t.V, tab_n * 4, hipMemcpyDeviceToHost, s);
  }
};

// The live nodes (state >= 2) of each of the T trees, numbered in heap order, into the layout gnx_model_desc takes: tree_off[0 .. T],
// left / right (-1 at a leaf).  on_split(q, slot) and on_leaf(q, slot) fill what else the trainer keeps for node q from table slot
// `slot`.  Returns the number of nodes.
template <class OnSplit, class OnLeaf>
inline int64_t gbt_compact_trees(const std::vector<int32_t>& hS, int64_t T, int32_t* tree_off, int32_t* left, int32_t* right, OnSplit on_split,
                                 OnLeaf on_leaf) {
  int64_t nn = 0;
  tree_off[0] = 0;
  for (int64_t t = 0; t < T; ++t) {
    const size_t o = (size_t)t * GBT_MAXN;
    int32_t idx[GBT_MAXN], cntn = 0;
    for (int node = 0; node < GBT_MAXN; ++node) idx[node] = (hS[o + node] >= 2) ? cntn++ : -1;
    for (int node = 0; node < GBT_MAXN; ++node) {
      if (hS[o + node] < 2) continue;
      const int64_t q = nn + idx[node];
      if (hS[o + node] == 2) {
        left[q] = idx[2 * node + 1]; right[q] = idx[2 * node + 2];
        on_split(q, o + node);
      } else {
        left[q] = -1; right[q] = -1;
        on_leaf(q, o + node);
      }
    }
    nn += cntn;
    tree_off[t + 1] = (int32_t)nn;
  }
  return nn;
}

}  // namespace
