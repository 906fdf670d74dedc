// forest/k_train_rforest.hip — training the random-forest BASE (RFBase) on gfx950: every window's
// RandomForestClassifier(n_estimators, max_depth).fit of scikit-learn 1.7.2, tree for tree.
//
// Replaces RFBase.train (reference src/Base/models.py:54-66 -> sklearn RandomForestClassifier(n_estimators=20, max_depth=4) per window,
// through Base.train_vectorized, src/Base/base.py:104-127).  The caller draws what numpy's generator decides (per tree the bootstrap
// row weights and the splitter's 32-bit state: gnomix_amd.train.rforest_bootstrap); everything after that is restated here and, in
// plain Python, in tests/rf_exact.py, which is held to live scikit-learn bit for bit.
//
// What a tree is (sklearn/tree/_tree.pyx DepthFirstTreeBuilder, _splitter.pyx node_split_best, _criterion.pyx Gini):
//  * a stack: the right child is pushed first, then the left; node ids are assigned in pop order;
//  * a popped node is a leaf without a search when depth >= max_depth or its impurity <= 2^-52; a leaf after the search when no
//    drawn column split it or improvement + 2^-52 < 0; a node that is a leaf before the search draws no random number;
//  * the search draws columns by Fisher-Yates over the tree-global `features` permutation (our_rand_r: xorshift 13 / 17 / 5, % 2^31;
//    rand_int(lo, hi) = lo + r % (hi - lo)) until max_features = max(1, int(sqrt(width))) were visited and one was not constant;
//    columns found constant in a node are remembered for its subtree (`constant_features`, n_constant_features inherited);
//  * a column's candidates lie between consecutive present codes, ascending: threshold 0.5 (or 1.0 when the node holds no 1), then
//    1.5; proxy = -wR impR - wL impL with imp = 1 - sum_k c_k^2 / (w w); strict >, the first best wins;
//  * improvement = (w / w_root) (imp - wR / w impR - wL / w impL).  All of it float64, one IEEE operation per step, in
//    scikit-learn's order (this file is compiled without contraction: no fused multiply-add).
//
// The search needs, per column, the node's weighted class counts for the codes 1 and 2 (code 0 = the node's class totals minus
// both).  The draw order is sequential inside a tree and independent across the W x n_trees trees, so the fit runs 2^max_depth - 1
// ROUNDS without host synchronisation; in round r every tree handles its r-th split search or idles.  Three launches per round:
//  1. k_rf_counts — per window ONE int8 matrix product (v_mfma_i32_16x16x64_i8), all columns of the window at once:
//       Out[(t, a), (v, f)] = sum_n L[(t, a), n] R[n, (v, f)],   L = weight[t, n] [y[n] = a] [row n sits in tree t's current node],
//       R = [X[n, f] = v], v in {1, 2}.  Sums are int32 and exact for weights <= 127 and N < 2^24.  Same tiling as k_lda_gram
//       (lda/k_train_lda.hip): 64 x 64 macro-tiles, 4 waves, both operands staged transposed in LDS with an 80-byte pitch;
//  2. k_rf_draw — one lane per tree walks node_split_best over the table, appends the node, pushes the children and pops until
//       the next node that needs a search (leaves met on the way are appended);
//  3. k_rf_partition — rows of the split node move to its left (X[n, feat] <= thr) or right child.
// Rows carry the heap index of their node (root 1, children 2 h and 2 h + 1).  The table is the raw int32 product; windows are
// processed in ranges that keep it under RF_TAB_BYTES.  No scratch, no atomics, no runtime-indexed register array, vector stores.
#include "../gnx_internal.h"
#include "../gnx_window.h"

#include <chrono>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int RF_T = 64;          // macro-tile edge
constexpr int RF_K = 64;          // rows of X per chunk = the MFMA's K
constexpr int RF_P = RF_K + 16;   // LDS row pitch, bytes (conflict-free 16-byte operand reads: lda/k_train_lda.hip)
constexpr int RF_ITEMS = 2 * RF_T * (RF_K / 4) / 256;
constexpr int RF_MAXA = 32;
constexpr int RF_STACK = 8;       // at most max_depth + 1 <= 6 records wait
constexpr size_t RF_TAB_BYTES = (size_t)512 << 20;
constexpr double RF_EPS = 2.220446049250313e-16;  // _tree.pyx EPSILON = np.finfo('double').eps

struct RfRec {
  int32_t heap, depth, parent, is_left, n_const, pad;
  double imp;
  int32_t c[RF_MAXA];  // weighted class counts of the node
};

struct RfTree {
  uint32_t rng;
  int32_t n_nodes, sp, active;   // active: stack[sp] is the node whose split search the next round runs
  int32_t split_heap, split_feat;  // this round's split for k_rf_partition (split_heap < 0: none)
  double split_thr;
  RfRec stack[RF_STACK];
};

struct RfGeom {
  const int8_t* X;
  const int32_t* Y;
  const uint8_t* wt;      // (W, T, N) bootstrap weights
  const uint32_t* state;  // (W, T) splitter states
  int64_t N, ldx, C, M, ctx;
  int32_t W, A, T, D, w0, nw, ldw, RP, cap;
  uint8_t* heap;      // [nw T][N]
  int32_t* tab;       // [nw][RP][2 ldw]
  uint16_t* feats;    // [nw T][ldw]
  uint16_t* cfeats;   // [nw T][ldw]
  RfTree* trees;      // [nw T]
  int32_t* o_left;    // [nw T][cap]
  int32_t* o_right;
  int32_t* o_feat;
  double* o_thr;
  double* o_val;      // [nw T][cap][A]
  int32_t* flag;      // != 0: a weight above 127
};

__device__ __forceinline__ double rf_gini(double sq, double w) { return 1.0 - sq / (w * w); }

// append the node of record r (children linked later), -> its id
__device__ __forceinline__ int rf_add_node(const RfGeom& G, RfTree* tr, size_t tree, const RfRec* r, bool leaf, int feat, double thr) {
  const int id = tr->n_nodes++;
  const size_t o = tree * G.cap;
  if (r->parent >= 0) (r->is_left ? G.o_left : G.o_right)[o + r->parent] = id;
  G.o_left[o + id] = -1;
  G.o_right[o + id] = -1;
  G.o_feat[o + id] = leaf ? 0 : feat;
  G.o_thr[o + id] = leaf ? -2.0 : thr;
  double w = 0.0;
  for (int a = 0; a < G.A; ++a) w += (double)r->c[a];
  for (int a = 0; a < G.A; ++a) G.o_val[(o + id) * G.A + a] = (double)r->c[a] / w;
  return id;
}

// pop until a node needs a split search (it stays at stack[sp]); leaves met on the way are appended
__device__ __forceinline__ void rf_advance(const RfGeom& G, RfTree* tr, size_t tree) {
  while (tr->sp > 0) {
    RfRec* r = &tr->stack[--tr->sp];
    if (r->depth >= G.D || r->imp <= RF_EPS) {
      rf_add_node(G, tr, tree, r, true, 0, 0.0);
      continue;
    }
    tr->active = 1;
    return;
  }
  tr->active = 0;
}

__global__ __launch_bounds__(64) void k_rf_init(RfGeom G) {
  const int64_t tree = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (tree >= (int64_t)G.nw * G.T) return;
  const int wl = (int)(tree / G.T), t = (int)(tree % G.T), w = G.w0 + wl;
  RfTree* tr = &G.trees[tree];
  const int width = (int)gnx_window_width(w, G.W, G.C, G.M, G.ctx);
  uint16_t* f = G.feats + (size_t)tree * G.ldw;
  uint16_t* cf = G.cfeats + (size_t)tree * G.ldw;
  for (int i = 0; i < G.ldw; ++i) {
    f[i] = (uint16_t)(i < width ? i : 0);
    cf[i] = 0;
  }
  RfRec* r = &tr->stack[0];
  for (int a = 0; a < RF_MAXA; ++a) r->c[a] = 0;
  const uint8_t* wt = G.wt + ((size_t)w * G.T + t) * G.N;
  int bad = 0;
  for (int64_t n = 0; n < G.N; ++n) {
    const int wn = wt[n];
    const int32_t y = G.Y[n * G.W + w];
    bad |= wn > 127;
    if (wn && y >= 0 && y < G.A) r->c[y] += wn;
  }
  if (bad) *G.flag = 1;
  double sq = 0.0, wsum = 0.0;
  for (int a = 0; a < G.A; ++a) {
    const double ck = (double)r->c[a];
    sq += ck * ck;
    wsum += ck;
  }
  r->heap = 1; r->depth = 0; r->parent = -1; r->is_left = 0; r->n_const = 0; r->pad = 0;
  r->imp = rf_gini(sq, wsum);
  tr->rng = G.state[(size_t)w * G.T + t];
  tr->n_nodes = 0;
  tr->sp = 1;
  tr->split_heap = -1; tr->split_feat = 0; tr->split_thr = 0.0;
  rf_advance(G, tr, (size_t)tree);
}

__global__ __launch_bounds__(256) void k_rf_counts(RfGeom G) {
  __shared__ __attribute__((aligned(16))) int8_t tz[2 * RF_T * RF_P];  // the (tree, class) rows, then the (code, column) columns
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wl = blockIdx.y, w = G.w0 + wl;
  const int width = (int)gnx_window_width(w, G.W, G.C, G.M, G.ctx);
  const int col0 = blockIdx.x * RF_T, row0 = blockIdx.z * RF_T;
  const int TA = G.T * G.A;
  if (col0 >= 2 * width) return;  // block-uniform, before any barrier (the last window is wider than the others)
  {
    int mine = 0;
    if (t < RF_T && row0 + t < TA) mine = G.trees[(size_t)wl * G.T + (row0 + t) / G.A].active;
    if (!__syncthreads_or(mine)) return;  // no tree of these rows searches in this round
  }
  // what each of this thread's staged items is.  Row side: tr >= 0 the tree (range-local), cls its class, hp the heap index of its
  // current node; column side: src the column of X, cls the code; tr < 0: zeros
  int32_t tr_[RF_ITEMS], cls_[RF_ITEMS], hp_[RF_ITEMS], src_[RF_ITEMS];
#pragma unroll
  for (int it = 0; it < RF_ITEMS; ++it) {
    const int idx = t + 256 * it;
    const int r = idx & 63;
    tr_[it] = -1; cls_[it] = 0; hp_[it] = 0; src_[it] = 0;
    if ((idx >> 10) == 0) {
      const int row = row0 + r;
      if (row < TA) {
        const int tl = wl * G.T + row / G.A;
        const RfTree* q = &G.trees[tl];
        if (q->active) {
          tr_[it] = tl;
          cls_[it] = row % G.A;
          hp_[it] = q->stack[q->sp].heap;
        }
      }
    } else {
      const int c = col0 + r;
      if (c < 2 * width) {
        const int v = c >= width ? 2 : 1;
        tr_[it] = 0;
        cls_[it] = v;
        src_[it] = (int32_t)gnx_pad_src((int64_t)w * G.M + (c - (v - 1) * width), G.C, G.ctx);
      }
    }
  }

  v4i acc[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = v4i{0, 0, 0, 0};
  const int8_t* ap = tz + (wv * 16 + (lane & 15)) * RF_P + (lane >> 4) * 16;
  const int8_t* bp = tz + (RF_T + (lane & 15)) * RF_P + (lane >> 4) * 16;

  for (int64_t k0 = 0; k0 < G.N; k0 += RF_K) {
#pragma unroll
    for (int it = 0; it < RF_ITEMS; ++it) {
      const int idx = t + 256 * it;
      const int g = (idx & 1023) >> 6;  // rows k0 + 4 g .. + 3
      uint32_t v = 0;
      if (tr_[it] >= 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t n = k0 + 4 * g + r;
          if (n < G.N) {
            uint32_t b;
            if ((idx >> 10) == 0) {
              const size_t o = (size_t)tr_[it] * G.N + n;
              b = (G.Y[n * G.W + w] == cls_[it] && G.heap[o] == hp_[it]) ? (uint32_t)G.wt[(size_t)G.w0 * G.T * G.N + o] : 0u;
            } else {
              b = (uint32_t)(G.X[n * G.ldx + src_[it]] == cls_[it]);
            }
            v |= b << (8 * r);
          }
        }
      }
      *reinterpret_cast<uint32_t*>(tz + ((idx >> 10) * RF_T + (idx & 63)) * RF_P + 4 * g) = v;
    }
    __syncthreads();
    const v4i a = *reinterpret_cast<const v4i*>(ap);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const v4i b = *reinterpret_cast<const v4i*>(bp + jt * 16 * RF_P);
      acc[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[jt], 0, 0, 0);
    }
    __syncthreads();
  }

  // C / D: column = lane & 15, row = 4 (lane >> 4) + reg.  Rows are all inside RP (a multiple of the macro-tile)
  int32_t* tw = G.tab + (size_t)wl * G.RP * 2 * G.ldw;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + wv * 16 + 4 * (lane >> 4) + r;
      const int c = col0 + jt * 16 + (lane & 15);
      if (c < 2 * width) {
        const int v = c >= width ? 2 : 1;
        tw[(size_t)row * 2 * G.ldw + (size_t)(v - 1) * G.ldw + (c - (v - 1) * width)] = acc[jt][r];
      }
    }
}

__device__ __forceinline__ int64_t rf_rand_int(uint32_t* s, int64_t lo, int64_t hi) {
  uint32_t x = *s;
  if (x == 0) x = 1;
  x ^= x << 13;
  x ^= x >> 17;
  x ^= x << 5;
  *s = x;
  return lo + (int64_t)(x & 0x7fffffffu) % (hi - lo);
}

__global__ __launch_bounds__(64) void k_rf_draw(RfGeom G) {
  const int64_t tree = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (tree >= (int64_t)G.nw * G.T) return;
  RfTree* tr = &G.trees[tree];
  tr->split_heap = -1;
  if (!tr->active) return;
  const int wl = (int)(tree / G.T), t = (int)(tree % G.T), w = G.w0 + wl, A = G.A;
  const int width = (int)gnx_window_width(w, G.W, G.C, G.M, G.ctx);
  const size_t ld2 = (size_t)2 * G.ldw;
  const int32_t* tb = G.tab + ((size_t)wl * G.RP + (size_t)t * A) * ld2;   // row a: tb + a ld2; code 1 at [f], code 2 at [ldw + f]
  uint16_t* F = G.feats + (size_t)tree * G.ldw;
  uint16_t* CF = G.cfeats + (size_t)tree * G.ldw;
  RfRec* rec = &tr->stack[tr->sp];
  const int heap = rec->heap, depth = rec->depth;
  const double imp = rec->imp;
  uint32_t rng = tr->rng;
  double wnode = 0.0;
  for (int a = 0; a < A; ++a) wnode += (double)rec->c[a];

  int max_features = (int)sqrt((double)width);  // max(1, int(sqrt(width))), whatever the last bit of the device's sqrt
  while ((max_features + 1) * (max_features + 1) <= width) ++max_features;
  while (max_features * max_features > width) --max_features;
  if (max_features < 1) max_features = 1;
  int f_i = width, n_visited = 0, n_found = 0, n_drawn = 0;
  const int n_known = rec->n_const;
  int n_total = n_known;
  double best_proxy = -INFINITY;
  int best_f = -1, best_cand = 0;
  double best_thr = 0.0;
  while (f_i > n_total && (n_visited < max_features || n_visited <= n_found + n_drawn)) {
    ++n_visited;
    int f_j = (int)rf_rand_int(&rng, n_drawn, f_i - n_found);
    if (f_j < n_known) {
      const uint16_t x = F[n_drawn]; F[n_drawn] = F[f_j]; F[f_j] = x;
      ++n_drawn;
      continue;
    }
    f_j += n_found;
    const int f = F[f_j];
    // weighted class counts by code; squares summed in class order as Gini.children_impurity does
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, sqL1 = 0.0, sqR1 = 0.0, sqL2 = 0.0, sqR2 = 0.0;
    for (int a = 0; a < A; ++a) {
      const int32_t c = rec->c[a], n1 = tb[a * ld2 + f], n2 = tb[a * ld2 + G.ldw + f], n0 = c - n1 - n2;
      t0 += (double)n0; t1 += (double)n1; t2 += (double)n2;
      const double l1 = (double)n0, r1 = (double)(c - n0), l2 = (double)(c - n2), r2 = (double)n2;
      sqL1 += l1 * l1; sqR1 += r1 * r1; sqL2 += l2 * l2; sqR2 += r2 * r2;
    }
    const bool p0 = t0 > 0.0, p1 = t1 > 0.0, p2 = t2 > 0.0;
    if ((int)p0 + (int)p1 + (int)p2 < 2) {
      const uint16_t x = F[f_j]; F[f_j] = F[n_total]; F[n_total] = x;
      ++n_found;
      ++n_total;
      continue;
    }
    --f_i;
    { const uint16_t x = F[f_i]; F[f_i] = F[f_j]; F[f_j] = x; }
    if (p0) {  // between code 0 and the next present code
      const double wL = t0, wR = wnode - t0;
      const double proxy = (-wR) * rf_gini(sqR1, wR) - wL * rf_gini(sqL1, wL);
      if (proxy > best_proxy) { best_proxy = proxy; best_f = f; best_cand = 1; best_thr = p1 ? 0.5 : 1.0; }
    }
    if (p1 && p2) {  // between the codes 1 and 2
      const double wR = t2, wL = wnode - t2;
      const double proxy = (-wR) * rf_gini(sqR2, wR) - wL * rf_gini(sqL2, wL);
      if (proxy > best_proxy) { best_proxy = proxy; best_f = f; best_cand = 2; best_thr = 1.5; }
    }
  }
  for (int i = 0; i < n_known; ++i) F[i] = CF[i];
  for (int i = 0; i < n_found; ++i) CF[n_known + i] = F[n_known + i];
  tr->rng = rng;
  rec->n_const = n_total;

  bool leaf = best_f < 0;
  double impL = 0.0, impR = 0.0;
  if (!leaf) {
    double sqL = 0.0, sqR = 0.0, wL = 0.0, wR = 0.0;
    for (int a = 0; a < A; ++a) {
      const int32_t c = rec->c[a], n1 = tb[a * ld2 + best_f], n2 = tb[a * ld2 + G.ldw + best_f];
      const int32_t L = best_cand == 1 ? c - n1 - n2 : c - n2;
      const double l = (double)L, r = (double)(c - L);
      sqL += l * l; sqR += r * r; wL += l; wR += r;
    }
    impL = rf_gini(sqL, wL);
    impR = rf_gini(sqR, wR);
    // weighted_n_samples = the tree's bootstrap weights = N
    const double improvement = (wnode / (double)G.N) * (imp - (wR / wnode * impR) - (wL / wnode * impL));
    leaf = improvement + RF_EPS < 0.0;
  }
  const int id = rf_add_node(G, tr, (size_t)tree, rec, leaf, best_f, best_thr);
  if (!leaf) {
    // right child into this record's slot (pushed first), left child above it
    RfRec* rr = rec;
    RfRec* rl = &tr->stack[tr->sp + 1];
    for (int a = 0; a < A; ++a) {
      const int32_t c = rec->c[a], n1 = tb[a * ld2 + best_f], n2 = tb[a * ld2 + G.ldw + best_f];
      const int32_t L = best_cand == 1 ? c - n1 - n2 : c - n2;
      rl->c[a] = L;
      rr->c[a] = c - L;
    }
    rr->heap = 2 * heap + 1; rr->depth = depth + 1; rr->parent = id; rr->is_left = 0; rr->n_const = n_total; rr->imp = impR;
    rl->heap = 2 * heap; rl->depth = depth + 1; rl->parent = id; rl->is_left = 1; rl->n_const = n_total; rl->imp = impL; rl->pad = 0;
    tr->sp += 2;
    tr->split_heap = heap; tr->split_feat = best_f; tr->split_thr = best_thr;
  }
  rf_advance(G, tr, (size_t)tree);
}

__global__ __launch_bounds__(256) void k_rf_partition(RfGeom G, int nb) {
  const int64_t tree = blockIdx.x / nb;
  const int64_t n = (int64_t)(blockIdx.x % nb) * 256 + threadIdx.x;
  const RfTree* tr = &G.trees[tree];
  const int h = tr->split_heap;
  if (h < 0 || n >= G.N) return;
  uint8_t* hp = G.heap + (size_t)tree * G.N + n;
  if (*hp != h) return;
  const int w = G.w0 + (int)(tree / G.T);
  const int64_t src = gnx_pad_src((int64_t)w * G.M + tr->split_feat, G.C, G.ctx);
  *hp = (uint8_t)(2 * h + ((double)G.X[n * G.ldx + src] <= tr->split_thr ? 0 : 1));
}

// per-phase wall times of the last timed run (gnx_train_rforest_phases): counts, draw, partition
bool g_rf_phases_on = false;
double g_rf_phase_ms[3] = {0, 0, 0};

int rforest_check(gnx_ctx* ctx, const void* X, const void* y, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t cx, int32_t A, int32_t T,
                  int32_t D, const void* wt, const void* st, const void* o1, const void* o2, const void* o3, const void* o4, const void* o5,
                  const void* o6, const void* o7, const void* o8) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (!X || !y || !wt || !st || !o1 || !o2 || !o3 || !o4 || !o5 || !o6 || !o7 || !o8) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: NULL pointer");
  if (A < 2 || A > RF_MAXA) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: A must be in [2, 32]");
  if (M <= 0 || C < M || cx < 0 || cx > C || C > ((int64_t)1 << 30)) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: bad C / M / ctx");
  if (N < 1 || ldx < C) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: bad N / ldx");
  if (N >= ((int64_t)1 << 24)) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: N reaches 2^24 (an int32 sum of 127 N weights could overflow)");
  if (T < 1 || T > 1024 || D < 1 || D > 5) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: 1 <= n_trees <= 1024, 1 <= max_depth <= 5");
  const int64_t W = C / M, ldw = M + 2 * cx + (C - M * W);
  if (ldw > 32768) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: windows wider than 32768 SNPs");
  if (W * T * (((int64_t)1 << (D + 1)) - 1) >= ((int64_t)1 << 31) || W * T * ((N + 255) / 256) >= ((int64_t)1 << 31))
    return gnx_fail(ctx, GNX_EINVAL, "train_rforest: problem too large for one launch sequence");
  return GNX_OK;
}

// dX (N, ldx) int8, dy (N, W) int32, dwt (W, T, N) uint8 and dstate (W, T) uint32 on the device; host outputs as in
// gnx_train_rforest (include/gnomix_hip.h).  *bad_weight = 1: a weight above 127 was met (the outputs are then meaningless)
hipError_t rforest_run(const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx, int32_t A, int32_t T,
                       int32_t D, const uint8_t* dwt, const uint32_t* dstate, int32_t* win_tree0, int32_t* tree_off, int32_t* left,
                       int32_t* right, int32_t* feat, double* thr, double* value, int64_t* n_nodes_out, int* bad_weight, hipStream_t s) {
  const int64_t W = C / M, ldw = M + 2 * cx + (C - M * W);
  const int RP = (int)(((int64_t)T * A + RF_T - 1) / RF_T) * RF_T, cap = (1 << (D + 1)) - 1, rounds = (1 << D) - 1;
  const size_t tab_w = (size_t)RP * 2 * ldw * 4;
  int64_t per = (int64_t)(RF_TAB_BYTES / tab_w);
  per = per < 1 ? 1 : per > W ? W : per > 65535 ? 65535 : per;
  const size_t TTm = (size_t)per * T;
  gnx_dev_tmp bHeap, bTab, bF, bCF, bTrees, bL, bR, bFe, bTh, bV, bFlag;
  GNX_HIPRET(bHeap.alloc(TTm * N));
  GNX_HIPRET(bTab.alloc((size_t)per * tab_w));
  GNX_HIPRET(bF.alloc(TTm * ldw * 2));
  GNX_HIPRET(bCF.alloc(TTm * ldw * 2));
  GNX_HIPRET(bTrees.alloc(TTm * sizeof(RfTree)));
  GNX_HIPRET(bL.alloc(TTm * cap * 4));
  GNX_HIPRET(bR.alloc(TTm * cap * 4));
  GNX_HIPRET(bFe.alloc(TTm * cap * 4));
  GNX_HIPRET(bTh.alloc(TTm * cap * 8));
  GNX_HIPRET(bV.alloc(TTm * cap * A * 8));
  GNX_HIPRET(bFlag.alloc(4));
  GNX_HIPRET(hipMemsetAsync(bFlag.p, 0, 4, s));

  const bool prof = g_rf_phases_on;
  double ms[3] = {0, 0, 0};
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

  std::vector<int32_t> hN, hL, hR, hF;
  std::vector<double> hT, hV;
  std::vector<RfTree> hTrees;
  int64_t nn = 0, tglob = 0;
  tree_off[0] = 0;
  const int nb = (int)((N + 255) / 256);
  for (int64_t w0 = 0; w0 < W; w0 += per) {
    const int64_t nw = W - w0 < per ? W - w0 : per;
    const size_t TT = (size_t)nw * T;
    RfGeom G{dX, dy, dwt, dstate, N, ldx, C, M, cx, (int32_t)W, A, T, D, (int32_t)w0, (int32_t)nw, (int32_t)ldw, RP, cap,
             bHeap.as<uint8_t>(), bTab.as<int32_t>(), bF.as<uint16_t>(), bCF.as<uint16_t>(), bTrees.as<RfTree>(), bL.as<int32_t>(),
             bR.as<int32_t>(), bFe.as<int32_t>(), bTh.as<double>(), bV.as<double>(), bFlag.as<int32_t>()};
    GNX_HIPRET(hipMemsetAsync(bHeap.p, 1, TT * N, s));
    hipLaunchKernelGGL(k_rf_init, dim3((unsigned)((TT + 63) / 64)), dim3(64), 0, s, G);
    GNX_HIPRET(hipGetLastError());
    phase(-1);
    for (int r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(k_rf_counts, dim3((unsigned)((2 * ldw + RF_T - 1) / RF_T), (unsigned)nw, (unsigned)(RP / RF_T)), dim3(256), 0, s, G);
      phase(0);
      hipLaunchKernelGGL(k_rf_draw, dim3((unsigned)((TT + 63) / 64)), dim3(64), 0, s, G);
      phase(1);
      if (r + 1 < rounds) hipLaunchKernelGGL(k_rf_partition, dim3((unsigned)(TT * nb)), dim3(256), 0, s, G, nb);
      GNX_HIPRET(hipGetLastError());
      phase(2);
    }
    // ---- this range's trees back to the host, packed in window and tree order ----
    hTrees.resize(TT); hL.resize(TT * cap); hR.resize(TT * cap); hF.resize(TT * cap); hT.resize(TT * cap); hV.resize(TT * cap * A);
    GNX_HIPRET(hipMemcpyAsync(hTrees.data(), bTrees.p, TT * sizeof(RfTree), hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(hL.data(), bL.p, TT * cap * 4, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(hR.data(), bR.p, TT * cap * 4, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(hF.data(), bFe.p, TT * cap * 4, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(hT.data(), bTh.p, TT * cap * 8, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipMemcpyAsync(hV.data(), bV.p, TT * cap * A * 8, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipStreamSynchronize(s));
    for (size_t t = 0; t < TT; ++t) {
      int32_t k = hTrees[t].n_nodes;
      if (k < 0 || k > cap || hTrees[t].active) return hipErrorUnknown;  // (cannot happen: a tree of depth D ends within 2^D - 1 searches)
      std::memcpy(left + nn, &hL[t * cap], (size_t)k * 4);
      std::memcpy(right + nn, &hR[t * cap], (size_t)k * 4);
      std::memcpy(feat + nn, &hF[t * cap], (size_t)k * 4);
      std::memcpy(thr + nn, &hT[t * cap], (size_t)k * 8);
      std::memcpy(value + nn * A, &hV[t * cap * A], (size_t)k * A * 8);
      nn += k;
      tree_off[++tglob] = (int32_t)nn;
    }
  }
  GNX_HIPRET(perr);
  int32_t flag = 0;
  GNX_HIPRET(hipMemcpyAsync(&flag, bFlag.p, 4, hipMemcpyDeviceToHost, s));
  GNX_HIPRET(hipStreamSynchronize(s));
  *bad_weight = flag;
  for (int64_t w = 0; w <= W; ++w) win_tree0[w] = (int32_t)(w * T);
  *n_nodes_out = nn;
  if (prof) std::memcpy(g_rf_phase_ms, ms, sizeof(ms));
  return hipSuccess;
}

}  // namespace

extern "C" {

int gnx_train_rforest_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx, int32_t A,
                          int32_t n_trees, int32_t max_depth, const uint8_t* d_weight, const uint32_t* d_state, int32_t* win_tree0,
                          int32_t* tree_off, int32_t* left, int32_t* right, int32_t* feat, double* thr, double* value, int64_t* n_nodes) {
  if (!ctx) return GNX_EINVAL;
  int rc = rforest_check(ctx, dX, dy, N, ldx, C, M, cx, A, n_trees, max_depth, d_weight, d_state, win_tree0, tree_off, left, right, feat, thr,
                         value, n_nodes);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  int bad = 0;
  HIPCHK(ctx, rforest_run(dX, N, ldx, dy, C, M, cx, A, n_trees, max_depth, d_weight, d_state, win_tree0, tree_off, left, right, feat, thr, value,
                          n_nodes, &bad, ctx->stream));
  if (bad) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: a bootstrap weight above 127 (the int8 operand of the count product)");
  return GNX_OK;
}

int gnx_train_rforest(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t cx, int32_t A,
                      int32_t n_trees, int32_t max_depth, const uint8_t* weight, const uint32_t* state, int32_t* win_tree0, int32_t* tree_off,
                      int32_t* left, int32_t* right, int32_t* feat, double* thr, double* value, int64_t* n_nodes) {
  if (!ctx) return GNX_EINVAL;
  int rc = rforest_check(ctx, X, y, N, ldx, C, M, cx, A, n_trees, max_depth, weight, state, win_tree0, tree_off, left, right, feat, thr, value,
                         n_nodes);
  if (rc != GNX_OK) return rc;
  const int64_t W = C / M;
  for (int64_t i = 0; i < N * W; ++i)
    if (y[i] < 0 || y[i] >= A) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: label outside [0, A)");
  for (int64_t n = 0; n < N; ++n)
    for (int64_t j = 0; j < C; ++j)
      if ((uint8_t)X[n * ldx + j] > 2) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: X holds a code outside {0, 1, 2}");
  const size_t wb = (size_t)W * n_trees * N, sb = (size_t)W * n_trees * 4;
  for (size_t i = 0; i < wb; ++i)
    if (weight[i] > 127) return gnx_fail(ctx, GNX_EINVAL, "train_rforest: a bootstrap weight above 127 (the int8 operand of the count product)");
  GNX_BIND_DEVICE(ctx);
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_x, (size_t)N * ldx + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, (size_t)N * W * 4)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, wb + 64 + sb)) != GNX_OK) return rc;
  uint8_t* dwt = (uint8_t*)ctx->ws_misc.p;
  uint32_t* dst = (uint32_t*)(dwt + ((wb + 63) / 64) * 64);
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_x.p, X, (size_t)(N - 1) * ldx + C, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, y, (size_t)N * W * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(dwt, weight, wb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(dst, state, sb, hipMemcpyHostToDevice, ctx->stream));
  int bad = 0;
  HIPCHK(ctx, rforest_run((const int8_t*)ctx->ws_x.p, N, ldx, (const int32_t*)ctx->ws_lab.p, C, M, cx, A, n_trees, max_depth, dwt, dst, win_tree0,
                          tree_off, left, right, feat, thr, value, n_nodes, &bad, ctx->stream));
  return GNX_OK;
}

int gnx_train_rforest_phases(int32_t enable, double* ms) {
  if (enable >= 0) g_rf_phases_on = enable != 0;
  if (ms) std::memcpy(ms, g_rf_phase_ms, sizeof(g_rf_phase_ms));
  return GNX_OK;
}

}  // extern "C"
