// k_train_gbt.hip — training the tree smoother on gfx950 (second half).
//
// Replaces Smoother.train of XGB_Smoother (reference src/Smooth/smooth.py:28-38 -> src/Smooth/models.py:14-20:
// XGBClassifier(n_estimators=100, max_depth=4, learning_rate=0.1, reg_lambda=1, objective='multi:softprob',
// num_class=A).fit(slide_window(B, S), y)).  xgboost is a third-party fitter that is not part of the reference tree, so what
// is rebuilt is the algorithm that call asks for — second-order boosting of A regression trees per round on the softmax
// objective — in the histogram form (xgboost's tree_method="hist"), MI355X-first:
//   * the (N*W, S*A) matrix of slide_window is never built: feature s*A + a of row (n, w) is byte (w+s)*A + a of the
//     haplotype's reflect-padded strip of 8-bit BINS (<= 256 quantile bins per class column, cut on a 1/65536 grid);
//   * gradients are rounded to multiples of 2^-30 and every sum is an int64, so histograms built with LDS atomics in any
//     order are exact: the result does not depend on scheduling, and the CPU oracle (gnxo_train_gbt under oracle/)
//     produces IDENTICAL trees — that is the parity test of this path (tests/test_train_gbt.py);
//   * all A trees of a round grow together, level by level: one histogram launch (block = a group of features x one class
//     x a slice of the rows, its 128 KB of LDS holding [feature][node][bin] sums) that visits only the rows of the SMALLER child of
//     every split (the sibling's histogram is parent - built, exact in int64), one split search (a wave per feature: prefix sums
//     over the bins, gains in float64, ties to the lowest feature then the lowest bin), one partition pass;
//   * the objective, the gain, the tie rule, the split commit and the leaf are forest/gnx_gbt_core.h's (shared with the base's trainer);
//     the softmax goes through det_exp (plain IEEE operations in a fixed order) because the oracle must reproduce p exactly.
// The trees come back in the layout gnx_model_desc takes (tree_off / left / right / feat / cond / tree_class), thresholds on
// the 1/65536 grid, so the trained smoother runs on k_smooth_xgb_rk like any other.
#include <algorithm>
#include <limits>
#include <cstring>
#include <numeric>
#include <thread>
#include <vector>

#include "gnx_internal.h"
#include "gnx_window.h"
#include "forest/gnx_gbt_core.h"

namespace {

constexpr int HIST_ENTRIES = 8192;     // (g, h) int64 pairs of LDS per histogram block = 128 KB

struct Geom {
  int64_t N, R;
  int32_t W, A, S, pad, Wp, F;
};

__device__ __forceinline__ int bucket_of(float v) {
  int b = (v > 0.0f) ? (int)(v * 65536.0f) : 0;
  return (v >= 1.0f) ? 65535 : b;
}

template <bool IS64>
__global__ __launch_bounds__(256) void k_gbt_cast_count(const void* B, float* Bf, uint32_t* cnt, Geom G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G.R * G.A) return;
  const float v = IS64 ? (float)reinterpret_cast<const double*>(B)[i] : reinterpret_cast<const float*>(B)[i];
  Bf[i] = v;
  atomicAdd(&cnt[(size_t)(i % G.A) * 65536 + bucket_of(v)], 1u);
}

__global__ __launch_bounds__(256) void k_gbt_quantise(const float* Bf, const uint8_t* lut, uint8_t* Bq, Geom G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= G.N * G.Wp * G.A) return;
  const int a = (int)(e % G.A);
  const int64_t nj = e / G.A;
  const int j = (int)(nj % G.Wp);
  const int64_t n = nj / G.Wp;
  const float v = Bf[(n * G.W + gnx_slide_src(j, G.W, G.pad)) * G.A + a];
  Bq[e] = lut[(size_t)a * 65536 + bucket_of(v)];
}

// one softmax per row for the A trees of the round; root sums per class; log loss (fixed point, informational)
template <int AMAX>
__global__ __launch_bounds__(256) void k_gbt_grad(const float* Fm, const int32_t* y, long long* gq, long long* hq, long long* rootG,
                                                   long long* rootH, long long* loss_fix, uint8_t* pos, int32_t* st, Geom G) {
  __shared__ long long sg[AMAX], sh[AMAX], sl;
  const int A = G.A;
  if (threadIdx.x < AMAX) { sg[threadIdx.x] = 0; sh[threadIdx.x] = 0; }
  if (threadIdx.x == 0) sl = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < G.R) {
    const double py = gbt_softprob_row<AMAX>(Fm + i * A, A, y[i], [&](int c, long long gi, long long hi) {
      gq[(size_t)c * G.R + i] = gi;
      hq[(size_t)c * G.R + i] = hi;
      pos[(size_t)c * G.R + i] = 0;
      atomicAdd(reinterpret_cast<unsigned long long*>(&sg[c]), (unsigned long long)gi);
      atomicAdd(reinterpret_cast<unsigned long long*>(&sh[c]), (unsigned long long)hi);
    });
    atomicAdd(reinterpret_cast<unsigned long long*>(&sl), (unsigned long long)llrint(-log(py > 1e-300 ? py : 1e-300) * 16777216.0));
  }
  __syncthreads();
  if (threadIdx.x < A) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&rootG[threadIdx.x * GBT_MAXN]), (unsigned long long)sg[threadIdx.x]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&rootH[threadIdx.x * GBT_MAXN]), (unsigned long long)sh[threadIdx.x]);
    st[threadIdx.x * GBT_MAXN] = 1;  // (every block writes the same value)
  }
  if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(loss_fix), (unsigned long long)sl);
}

// histograms of one level for all classes: block = (feature group, class, row slice); LDS [feature][node of level][bin] (g, h)
constexpr int HIST_T = 1024;  // one block per CU (its histogram fills the LDS): 16 waves keep enough row loads in flight
__global__ __launch_bounds__(HIST_T) void k_gbt_hist(const uint8_t* Bq, const long long* gq, const long long* hq, const uint8_t* pos,
                                                   const int32_t* st, const int32_t* build, long long* part, int d, int fpb, int n_slices, Geom G) {
  extern __shared__ __attribute__((aligned(16))) long long sh[];
  const int nl = 1 << d, base = nl - 1;
  const int f0 = blockIdx.x * fpb, c = blockIdx.y, slice = blockIdx.z;
  const int nf = min(fpb, G.F - f0);
  // two planes, [feature][node][bin] of g and the same of h: 8-byte cells, so the 64 lanes of an atomic spread over 32 bank pairs
  // (16-byte (g, h) cells would leave 16: a 4-way conflict at best)
  const int cells = fpb * nl * 256;
  unsigned long long* shg = reinterpret_cast<unsigned long long*>(sh);
  unsigned long long* shh = shg + cells;
  for (int e = threadIdx.x; e < 2 * cells; e += HIST_T) sh[e] = 0;
  __syncthreads();
  const int64_t r0 = G.R * slice / n_slices, r1 = G.R * (slice + 1) / n_slices;
  const uint8_t* posc = pos + (size_t)c * G.R;
  const int32_t* stc = st + c * GBT_MAXN;
  const int32_t* bldc = build + c * GBT_MAXN;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += HIST_T) {
    const int node = posc[i], k = node - base;
    if (k < 0 || k >= nl || stc[node] != 1 || !bldc[node]) continue;  // (the sibling of a built node is derived: parent - built)
    const int64_t n = i / G.W;
    const int w = (int)(i - n * G.W);
    const unsigned long long g = (unsigned long long)gq[(size_t)c * G.R + i], h = (unsigned long long)hq[(size_t)c * G.R + i];
    const uint8_t* q = Bq + ((size_t)n * G.Wp + w) * G.A + f0;
    for (int f4 = 0; f4 < nf; f4 += 4) {  // four bins per (unaligned) dword load; bytes past the block's features are not used
      uint32_t qv;
      __builtin_memcpy(&qv, q + f4, 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (f4 + u < nf) {
          const int cell = ((f4 + u) * nl + k) * 256 + (int)((qv >> (8 * u)) & 0xffu);
          atomicAdd(shg + cell, g);
          atomicAdd(shh + cell, h);
        }
      }
    }
  }
  __syncthreads();
  // part[slice][c][k][f][bin][2]
  for (int e = threadIdx.x; e < nf * nl * 256; e += HIST_T) {
    const int fi = e / (nl * 256), r = e - fi * nl * 256, k = r / 256, b = r - k * 256;
    long long* dst = part + ((((size_t)slice * G.A + c) * nl + k) * G.F + (f0 + fi)) * 512 + b * 2;
    dst[0] = (long long)shg[e];
    dst[1] = (long long)shh[e];
  }
}

struct Best {
  double gain;
  int f, j;
  long long GL, HL;
};
constexpr int SPLIT_CHUNKS = 16;// the features of a node are searched by this many blocks; k_gbt_split_pick takes the best of them

// best split of every open node of the level: grid (node of level, class, feature chunk); a wave per feature, lanes over the bins
__global__ __launch_bounds__(256) void k_gbt_split(const long long* part, const int32_t* ncut, const long long* nG, const long long* nH,
                                                    const int32_t* st, const int32_t* build, const long long* Hprev, long long* Hcur, Best* cand, int d,
                                                    int n_slices, double lambda, double gamma, double mcw, Geom G) {
  const int nl = 1 << d, base = nl - 1;
  const int k = blockIdx.x, c = blockIdx.y, node = base + k;
  if (st[c * GBT_MAXN + node] != 1) return;
  const int fchunk = (G.F + SPLIT_CHUNKS - 1) / SPLIT_CHUNKS, fbeg = blockIdx.z * fchunk, fend = min(G.F, fbeg + fchunk);
  const bool built = build[c * GBT_MAXN + node] != 0;
  const int ks = built ? k : (k ^ 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long Gn = nG[c * GBT_MAXN + node], Hn = nH[c * GBT_MAXN + node];
  const double root_term = gbt_root_term(Gn, Hn, lambda);
  // the running best as scalars (see gbt_block_best: no struct selects); a candidate exists iff bf >= 0
  double bg = gbt_gain_floor(gamma);
  int bf = -1, bj = -1;
  long long bGL = 0, bHL = 0;
  for (int f = fbeg + wave; f < fend; f += 4) {
    const int nc = ncut[f % G.A];
    long long g4[4], h4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { g4[q] = 0; h4[q] = 0; }
    for (int s = 0; s < n_slices; ++s) {
      const long long* src = part + ((((size_t)s * G.A + c) * nl + ks) * G.F + f) * 512 + lane * 8;
#pragma unroll
      for (int q = 0; q < 4; ++q) { g4[q] += src[q * 2]; h4[q] += src[q * 2 + 1]; }
    }
    if (!built) {  // sibling subtraction: this node's histogram = its parent's - its (built) sibling's, exact in int64
      const long long* par = Hprev + (((size_t)c * (nl >> 1) + (k >> 1)) * G.F + f) * 512 + lane * 8;
#pragma unroll
      for (int q = 0; q < 4; ++q) { g4[q] = par[q * 2] - g4[q]; h4[q] = par[q * 2 + 1] - h4[q]; }
    }
    {
      long long* dst = Hcur + (((size_t)c * nl + k) * G.F + f) * 512 + lane * 8;
#pragma unroll
      for (int q = 0; q < 4; ++q) { dst[q * 2] = g4[q]; dst[q * 2 + 1] = h4[q]; }
    }
    // inclusive prefix over the 256 bins: inside the lane, then across lanes
#pragma unroll
    for (int q = 1; q < 4; ++q) { g4[q] += g4[q - 1]; h4[q] += h4[q - 1]; }
    long long og = g4[3], oh = h4[3];
    for (int o = 1; o < 64; o <<= 1) {
      const long long tg = __shfl_up(og, o), th = __shfl_up(oh, o);
      if (lane >= o) { og += tg; oh += th; }
    }
    const long long eg = og - g4[3], eh = oh - h4[3];  // exclusive prefix of this lane
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane * 4 + q;
      if (j >= nc) continue;
      const long long GL = eg + g4[q], HL = eh + h4[q];
      double gain;
      if (!gbt_split_gain(GL, HL, Gn, Hn, root_term, lambda, mcw, &gain)) continue;
      if (bf < 0 ? gain > bg : gbt_beats(gain, f, j, bg, bf, bj)) { bg = gain; bf = f; bj = j; bGL = GL; bHL = HL; }
    }
  }
  gbt_block_best(bg, bf, bj, bGL, bHL);
  if (threadIdx.x == 0) {
    Best* dst = cand + ((size_t)c * nl + k) * SPLIT_CHUNKS + blockIdx.z;
    dst->gain = bg; dst->f = bf; dst->j = bj; dst->GL = bGL; dst->HL = bHL;
  }
}

__global__ void k_gbt_split_pick(const Best* cand, GbtTables t, int d, int A) {
  const int nl = 1 << d, base = nl - 1;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= A * nl) return;
  const int c = e / nl, k = e - c * nl, node = base + k, o = c * GBT_MAXN;
  if (t.S[o + node] != 1) return;
  const Best* cq = cand + (size_t)e * SPLIT_CHUNKS;  // (scalars, not struct copies: see gbt_block_best)
  int bf = -1, bj = -1;
  double bg = 0.0;
  long long bGL = 0, bHL = 0;
  for (int q = 0; q < SPLIT_CHUNKS; ++q) {
    const double tg = cq[q].gain;
    const int tf = cq[q].f, tj = cq[q].j;
    if (tf < 0) continue;
    if (bf < 0 || gbt_beats(tg, tf, tj, bg, bf, bj)) { bg = tg; bf = tf; bj = tj; bGL = cq[q].GL; bHL = cq[q].HL; }
  }
  gbt_commit_split(t, o, node, bf >= 0, bf, bj, bGL, bHL);
}

__global__ __launch_bounds__(256) void k_gbt_partition(const uint8_t* Bq, uint8_t* pos, const int32_t* st, const int32_t* nF, const int32_t* nB,
                                                        int32_t* cnt, int d, Geom G) {
  __shared__ int lc[64];
  if (threadIdx.x < 64) lc[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i < G.R) {
    const int node = pos[(size_t)c * G.R + i];
    if (node >= (1 << d) - 1 && st[c * GBT_MAXN + node] == 2) {
      const int64_t n = i / G.W;
      const int w = (int)(i - n * G.W);
      const uint8_t q = Bq[((size_t)n * G.Wp + w) * G.A + nF[c * GBT_MAXN + node]];
      const int child = q <= nB[c * GBT_MAXN + node] ? 2 * node + 1 : 2 * node + 2;
      pos[(size_t)c * G.R + i] = (uint8_t)child;
      atomicAdd(&lc[child], 1);  // rows per child: the smaller child of a pair gets its histogram built, the other derived
    }
  }
  __syncthreads();
  if (threadIdx.x < GBT_MAXN && lc[threadIdx.x]) atomicAdd(&cnt[c * GBT_MAXN + threadIdx.x], lc[threadIdx.x]);
}

// which child of every node split at level d gets its histogram built at level d + 1 (the one with fewer rows; ties: the left)
__global__ void k_gbt_choose(const int32_t* st, const int32_t* cnt, int32_t* build, int d, int A) {
  const int nl = 1 << d, base = nl - 1;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= A * nl) return;
  const int c = e / nl, node = base + (e - c * nl), o = c * GBT_MAXN;
  if (st[o + node] != 2) return;
  const int l = 2 * node + 1, r = 2 * node + 2;
  const bool left = cnt[o + l] <= cnt[o + r];
  build[o + l] = left ? 1 : 0;
  build[o + r] = left ? 0 : 1;
}

__global__ void k_gbt_close(GbtTables t, int A, double eta, double lambda) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < A * GBT_MAXN) gbt_close_node(t, e, eta, lambda);
}

__global__ __launch_bounds__(256) void k_gbt_margin(float* Fm, const uint8_t* pos, const float* nV, Geom G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= G.R * G.A) return;
  const int c = (int)(e % G.A);
  const int64_t i = e / G.A;
  Fm[e] += nV[c * GBT_MAXN + pos[(size_t)c * G.R + i]];
}

// ---- exact greedy (gnx_gbt_params::tree_method = 1) ------------------------------------------------------------------------------
// xgboost's tree_method="exact" (what XGBClassifier(...) of src/Smooth/models.py:14-20 uses for data of this size; ColMaker's column
// scan restated, NOT pinned to xgboost: absent from the image): per node and feature the node's rows in ascending feature value,
// a candidate between every two consecutive DISTINCT values v0 < v1: rows up to v0 left, threshold (v0 + v1) * 0.5f (v1 when that
// rounds down to v0).  All features s*A + a of one class column a read the same values — the haplotypes' padded strips of that column —
// so ONE sorted list of strip positions per column (sorted on the host once per training) serves its S features: feature s sees
// position (n, j) as row (n, j - s).  k_gbt_exact_scan: one wave per (feature, class tree), 64 sorted positions per step; for every
// node present in the step a masked wave scan gives each of its rows the node's sums before it and the previous value of the node
// (the last row of an earlier step is carried in LDS); gains in float64 from exact int64 sums, first-best-wins in scan order — the
// CPU oracle (gnxo_train_gbt, tree_method 1: a qsort per node and feature) grows IDENTICAL trees (tests/test_train_gbt.py).
struct ExBest {
  double gain;   // < 0: no admissible split of this node on this feature
  float thr;
  int32_t pad_;
  long long GL, HL;
};

__device__ __forceinline__ float gbt_mid(float v0, float v1) {
  const float m = (v0 + v1) * 0.5f;
  return m > v0 ? m : v1;
}

__global__ __launch_bounds__(64) void k_gbt_exact_scan(const int32_t* __restrict__ ordn, const int32_t* __restrict__ ordj, const float* __restrict__ val,
                                                      const long long* __restrict__ gq, const long long* __restrict__ hq, const uint8_t* __restrict__ pos,
                                                      const int32_t* __restrict__ st, const long long* __restrict__ nG, const long long* __restrict__ nH,
                                                      ExBest* __restrict__ cand, int d, double lambda, double gamma, double mcw, Geom G) {
  __shared__ long long accG[32], accH[32], bGL[32], bHL[32], nodeG[32], nodeH[32];
  __shared__ double bgain[32];
  __shared__ float lastv[32], bthr[32];
  __shared__ int seen[32], open_[32], found[32];
  const int nl = 1 << d, base = nl - 1, lane = threadIdx.x;
  const int f = blockIdx.x, c = blockIdx.y, sft = f / G.A, a = f - sft * G.A;
  if (lane < nl) {
    const int node = base + lane;
    accG[lane] = 0; accH[lane] = 0; seen[lane] = 0; found[lane] = 0;
    open_[lane] = st[c * GBT_MAXN + node] == 1;
    nodeG[lane] = nG[c * GBT_MAXN + node]; nodeH[lane] = nH[c * GBT_MAXN + node];
    bgain[lane] = gbt_gain_floor(gamma);
  }
  __syncthreads();
  const int64_t NP = G.N * G.Wp, col = (int64_t)a * NP;
  const long long* gc = gq + (size_t)c * G.R;
  const long long* hc = hq + (size_t)c * G.R;
  const uint8_t* pc = pos + (size_t)c * G.R;
  for (int64_t p0 = 0; p0 < NP; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool in = p < NP;
    const int n = in ? ordn[col + p] : 0, j = in ? ordj[col + p] : 0;
    const float v = in ? val[col + p] : 0.f;
    const int w = j - sft;
    const bool valid = in && w >= 0 && w < G.W;
    const int64_t row = valid ? (int64_t)n * G.W + w : 0;
    const int k = valid ? (int)pc[row] - base : -1;
    const bool live = valid && k >= 0 && k < nl && open_[k];
    const long long g = live ? gc[row] : 0, h = live ? hc[row] : 0;
    unsigned long long rem = __ballot(live);
    while (rem) {
      const int kcur = __shfl(k, __builtin_ctzll(rem));
      const bool mask = live && k == kcur;
      const unsigned long long bal = __ballot(mask);
      rem &= ~bal;
      long long sg = mask ? g : 0, sh = mask ? h : 0;
      const long long ig = sg, ih = sh;
      for (int o = 1; o < 64; o <<= 1) {
        const long long tg = __shfl_up(sg, o), th = __shfl_up(sh, o);
        if (lane >= o) { sg += tg; sh += th; }
      }
      const unsigned long long below = bal & ((1ull << lane) - 1ull);
      bool hasp = below != 0;
      float vp = __shfl(v, hasp ? 63 - __builtin_clzll(below) : 0);
      if (!hasp) { vp = lastv[kcur]; hasp = seen[kcur] != 0; }
      bool ok = false;
      double gain = 0.0;
      long long GL = 0, HL = 0;
      if (mask && hasp && vp < v) {
        GL = accG[kcur] + (sg - ig);
        HL = accH[kcur] + (sh - ih);
        const long long Gn = nodeG[kcur], Hn = nodeH[kcur];
        // strictly better than every earlier candidate of this node on this feature
        ok = gbt_split_gain(GL, HL, Gn, Hn, gbt_root_term(Gn, Hn, lambda), lambda, mcw, &gain) && gain > bgain[kcur];
      }
      const unsigned long long cb = __ballot(ok);
      if (cb) {  // the largest gain of the step, the earliest lane among equals
        double mx = ok ? gain : -1.0;
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        const int win = __builtin_ctzll(__ballot(ok && gain == mx));
        if (lane == win) { bgain[kcur] = gain; bthr[kcur] = gbt_mid(vp, v); bGL[kcur] = GL; bHL[kcur] = HL; found[kcur] = 1; }
      }
      if (lane == 63 - __builtin_clzll(bal)) { accG[kcur] += sg; accH[kcur] += sh; lastv[kcur] = v; seen[kcur] = 1; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __syncthreads();
  if (lane < nl) {
    ExBest* dst = cand + ((size_t)c * nl + lane) * G.F + f;
    dst->gain = found[lane] ? bgain[lane] : -1.0;
    dst->thr = bthr[lane];
    dst->pad_ = 0;
    dst->GL = bGL[lane];
    dst->HL = bHL[lane];
  }
}

// best feature of every open node: features in ascending order, strictly larger gain replaces (first best wins)
__global__ void k_gbt_exact_pick(const ExBest* cand, GbtTables t, int d, int A, int F) {
  const int nl = 1 << d, base = nl - 1;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= A * nl) return;
  const int c = e / nl, k = e - c * nl, node = base + k, o = c * GBT_MAXN;
  if (t.S[o + node] != 1) return;
  const ExBest* cq = cand + (size_t)e * F;
  int bf = -1;
  double bg = 0.0;
  for (int f = 0; f < F; ++f) {
    const double tg = cq[f].gain;
    if (tg < 0.0) continue;
    if (bf < 0 || tg > bg) { bf = f; bg = tg; }
  }
  if (bf < 0) { gbt_commit_split(t, o, node, false, 0, 0, 0, 0); return; }
  gbt_commit_split(t, o, node, true, bf, __float_as_int(cq[bf].thr), cq[bf].GL, cq[bf].HL);  // (the threshold's bits where the histogram form keeps a bin)
}

__global__ __launch_bounds__(256) void k_gbt_exact_partition(const float* Bf, uint8_t* pos, const int32_t* st, const int32_t* nF, const int32_t* nB, int d, Geom G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= G.R) return;
  const int node = pos[(size_t)c * G.R + i];
  if (node >= (1 << d) - 1 && st[c * GBT_MAXN + node] == 2) {
    const int64_t n = i / G.W;
    const int w = (int)(i - n * G.W);
    const int f = nF[c * GBT_MAXN + node], sft = f / G.A, a = f - sft * G.A;
    const float v = Bf[(n * G.W + gnx_slide_src(w + sft, G.W, G.pad)) * G.A + a];
    pos[(size_t)c * G.R + i] = (uint8_t)(v < __int_as_float(nB[c * GBT_MAXN + node]) ? 2 * node + 1 : 2 * node + 2);
  }
}

}  // namespace

// dB (N, W, A) float32 / float64 and dy (N, W) int32 on the device.  Host outputs as in gnx_train_gbt (include/gnomix_hip.h).
hipError_t gnx_train_gbt_run(const void* dB, int b_is_f64, const int32_t* dy, int64_t N, int32_t W, int32_t A, int32_t S,
                             const gnx_gbt_params& P, int32_t* tree_off, int32_t* tree_class, int32_t* left, int32_t* right,
                             int32_t* feat, float* cond, int64_t* n_nodes_out, double* loss_out, int n_cu, hipStream_t s) {
  Geom G;
  G.N = N; G.W = W; G.A = A; G.S = S; G.pad = (S + 1) / 2; G.Wp = W + 2 * G.pad; G.F = S * A; G.R = N * (int64_t)W;
  const int D = P.max_depth, T = P.n_rounds * A;
  const int64_t RA = G.R * A;
  gnx_dev_tmp bBf, bCnt, bLut, bBq, bFm, bG, bH, bPos, bPart, bTab, bNcut, bLoss, bCand, bRows, bLev;
  GNX_HIPRET(bBf.alloc((size_t)RA * 4));
  GNX_HIPRET(bCnt.alloc((size_t)A * 65536 * 4));
  GNX_HIPRET(bLut.alloc((size_t)A * 65536));
  GNX_HIPRET(bBq.alloc((size_t)N * G.Wp * A + 64));
  GNX_HIPRET(bFm.alloc((size_t)RA * 4));
  GNX_HIPRET(bG.alloc((size_t)RA * 8));
  GNX_HIPRET(bH.alloc((size_t)RA * 8));
  GNX_HIPRET(bPos.alloc((size_t)RA));
  GNX_HIPRET(bNcut.alloc((size_t)A * 4));
  GNX_HIPRET(bLoss.alloc((size_t)(P.n_rounds + 1) * 8));
  GNX_HIPRET(bCand.alloc((size_t)A * 32 * SPLIT_CHUNKS * sizeof(Best)));
  const size_t tab_n = (size_t)T * GBT_MAXN;  // node tables of every tree, and one more round's that the last loss pass writes unread
  GbtTables tab;
  GNX_HIPRET(gbt_tables_alloc(bTab, tab, tab_n + (size_t)A * GBT_MAXN, s));
  GNX_HIPRET(hipMemsetAsync(bCnt.p, 0, (size_t)A * 65536 * 4, s));
  GNX_HIPRET(hipMemsetAsync(bLoss.p, 0, (size_t)(P.n_rounds + 1) * 8, s));

  // ---- cuts ----
  const unsigned gRA = (unsigned)((RA + 255) / 256);
  if (b_is_f64) hipLaunchKernelGGL(k_gbt_cast_count<true>, dim3(gRA), dim3(256), 0, s, dB, bBf.as<float>(), bCnt.as<uint32_t>(), G);
  else hipLaunchKernelGGL(k_gbt_cast_count<false>, dim3(gRA), dim3(256), 0, s, dB, bBf.as<float>(), bCnt.as<uint32_t>(), G);
  GNX_HIPRET(hipGetLastError());
  std::vector<uint32_t> cnt((size_t)A * 65536);
  GNX_HIPRET(hipMemcpyAsync(cnt.data(), bCnt.p, cnt.size() * 4, hipMemcpyDeviceToHost, s));
  GNX_HIPRET(hipStreamSynchronize(s));
  std::vector<float> cuts((size_t)A * 256, 0.f);
  std::vector<int32_t> ncut((size_t)A, 0);
  std::vector<uint8_t> lut((size_t)A * 65536);
  for (int a = 0; a < A; ++a) {  // the k-th cut is the upper edge of the first bucket whose cumulative count reaches k*R/max_bin
    int k = 1, nc = 0;
    uint64_t cum = 0;
    for (int u = 0; u < 65536 && k < P.max_bin; ++u) {
      cum += cnt[(size_t)a * 65536 + u];
      bool hit = false;
      while (k < P.max_bin && cum >= (uint64_t)k * (uint64_t)G.R / (uint64_t)P.max_bin) { ++k; hit = true; }
      if (hit && u < 65535) cuts[(size_t)a * 256 + nc++] = (float)(u + 1) / 65536.0f;
    }
    ncut[(size_t)a] = nc;
    int c = 0;
    for (int u = 0; u < 65536; ++u) {
      while (c < nc && (int)(cuts[(size_t)a * 256 + c] * 65536.0f) <= u) ++c;
      lut[(size_t)a * 65536 + u] = (uint8_t)c;
    }
  }
  GNX_HIPRET(hipMemcpyAsync(bLut.p, lut.data(), lut.size(), hipMemcpyHostToDevice, s));
  GNX_HIPRET(hipMemcpyAsync(bNcut.p, ncut.data(), (size_t)A * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_gbt_quantise, dim3((unsigned)((N * G.Wp * A + 255) / 256)), dim3(256), 0, s, bBf.as<float>(), bLut.as<uint8_t>(),
                     bBq.as<uint8_t>(), G);
  hipLaunchKernelGGL(k_gbt_fill, dim3(gRA), dim3(256), 0, s, bFm.as<float>(), (float)P.base_score, RA);
  GNX_HIPRET(hipGetLastError());

  // ---- exact greedy: one sorted list of padded strip positions per class column (host sort, once per training) ----
  const bool exact = P.tree_method == 1;
  gnx_dev_tmp bOrdN, bOrdJ, bVal, bEx;
  if (exact) {
    const int64_t NP = N * G.Wp;
    std::vector<float> hB((size_t)RA);
    GNX_HIPRET(hipMemcpyAsync(hB.data(), bBf.p, (size_t)RA * 4, hipMemcpyDeviceToHost, s));
    GNX_HIPRET(hipStreamSynchronize(s));
    std::vector<int32_t> on((size_t)A * NP), oj((size_t)A * NP);
    std::vector<float> ov((size_t)A * NP);
    auto sort_col = [&](int a) {
      std::vector<float> v((size_t)NP);
      for (int64_t n = 0; n < N; ++n)
        for (int64_t j = 0; j < G.Wp; ++j) {
          const int64_t src = j < G.pad ? G.pad - 1 - j : (j < G.pad + W ? j - G.pad : W - 1 - (j - G.pad - W));
          const float f = hB[(size_t)((n * W + src) * A + a)];
          v[(size_t)(n * G.Wp + j)] = f == f ? f : std::numeric_limits<float>::infinity();  // a NaN would break the comparator's strict weak order
        }
      std::vector<int32_t> idx((size_t)NP);
      std::iota(idx.begin(), idx.end(), 0);
      std::sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return v[(size_t)x] < v[(size_t)y] || (v[(size_t)x] == v[(size_t)y] && x < y); });
      for (int64_t p = 0; p < NP; ++p) {
        const int32_t q = idx[(size_t)p];
        on[(size_t)a * NP + p] = (int32_t)(q / G.Wp);
        oj[(size_t)a * NP + p] = (int32_t)(q % G.Wp);
        ov[(size_t)a * NP + p] = v[(size_t)q];
      }
    };
    {
      std::vector<std::thread> th;
      for (int a = 0; a < A; ++a) {
        try { th.emplace_back(sort_col, a); } catch (...) { sort_col(a); }
      }
      for (auto& t : th) t.join();
    }
    GNX_HIPRET(bOrdN.alloc((size_t)A * NP * 4));
    GNX_HIPRET(bOrdJ.alloc((size_t)A * NP * 4));
    GNX_HIPRET(bVal.alloc((size_t)A * NP * 4));
    GNX_HIPRET(bEx.alloc((size_t)A * 16 * G.F * sizeof(ExBest)));
    GNX_HIPRET(hipMemcpyAsync(bOrdN.p, on.data(), (size_t)A * NP * 4, hipMemcpyHostToDevice, s));
    GNX_HIPRET(hipMemcpyAsync(bOrdJ.p, oj.data(), (size_t)A * NP * 4, hipMemcpyHostToDevice, s));
    GNX_HIPRET(hipMemcpyAsync(bVal.p, ov.data(), (size_t)A * NP * 4, hipMemcpyHostToDevice, s));
    GNX_HIPRET(hipStreamSynchronize(s));   // (the host vectors leave scope)
  }

  // ---- histogram geometry per level: features per block from the LDS budget, row slices to fill the chip ----
  int fpb[8], nsl[8];
  size_t part_entries = 0;
  for (int d = 0; d < D; ++d) {
    const int nl = 1 << d;
    fpb[d] = std::max(1, HIST_ENTRIES / (nl * 256));
    fpb[d] = std::min(fpb[d], (int)G.F);
    const int fg = (G.F + fpb[d] - 1) / fpb[d];
    int ns = (int)std::max<int64_t>(1, ((int64_t)8 * n_cu + (int64_t)fg * A - 1) / ((int64_t)fg * A));
    ns = (int)std::min<int64_t>(ns, std::max<int64_t>(1, G.R / 1024));
    nsl[d] = ns;
    part_entries = std::max(part_entries, (size_t)ns * A * nl * G.F * 512);
  }
  GNX_HIPRET(bPart.alloc(part_entries * 8));
  // rows per node and "build this node's histogram" flags of the round's trees; the level's summed histograms, this level's and the
  // previous one's (a derived node reads its parent's)
  GNX_HIPRET(bRows.alloc((size_t)2 * A * GBT_MAXN * 4));
  int32_t* dCnt = bRows.as<int32_t>();
  int32_t* dBuild = dCnt + (size_t)A * GBT_MAXN;
  const size_t lev_entries = (size_t)A * ((size_t)1 << (D - 1)) * G.F * 512;
  GNX_HIPRET(bLev.alloc(2 * lev_entries * 8));
  GNX_LDS_OPTIN((size_t)HIST_ENTRIES * 16, k_gbt_hist);

  const unsigned gR = (unsigned)((G.R + 255) / 256);
  // gradients before round r: root sums and open roots into (rG, rH, rS), the loss into slot r
  auto grad = [&](int r, long long* rG, long long* rH, int32_t* rS) {
#define GBT_GRAD(AM) hipLaunchKernelGGL(k_gbt_grad<AM>, dim3(gR), dim3(256), 0, s, bFm.as<float>(), dy, bG.as<long long>(), bH.as<long long>(), rG, rH, \
                                        bLoss.as<long long>() + r, bPos.as<uint8_t>(), rS, G)
    if (A <= 8) GBT_GRAD(8);
    else if (A <= 16) GBT_GRAD(16);
    else GBT_GRAD(32);
#undef GBT_GRAD
  };
  for (int r = 0; r < P.n_rounds; ++r) {
    const GbtTables rt = tab.at((size_t)r * A * GBT_MAXN);  // the round's A trees
    grad(r, rt.G, rt.H, rt.S);
    GNX_HIPRET(hipMemsetAsync(dCnt, 0, (size_t)A * GBT_MAXN * 4, s));
    GNX_HIPRET(hipMemsetAsync(dBuild, 0xff, (size_t)A * GBT_MAXN * 4, s));  // (the roots are built; children are decided by k_gbt_choose)
    for (int d = 0; exact && d < D; ++d) {
      const int nl = 1 << d;
      hipLaunchKernelGGL(k_gbt_exact_scan, dim3((unsigned)G.F, (unsigned)A), dim3(64), 0, s, bOrdN.as<int32_t>(), bOrdJ.as<int32_t>(), bVal.as<float>(),
                         bG.as<long long>(), bH.as<long long>(), bPos.as<uint8_t>(), rt.S, rt.G, rt.H, bEx.as<ExBest>(), d, P.lambda, P.gamma, P.min_child_weight, G);
      hipLaunchKernelGGL(k_gbt_exact_pick, dim3((unsigned)((A * nl + 63) / 64)), dim3(64), 0, s, bEx.as<ExBest>(), rt, d, A, (int)G.F);
      hipLaunchKernelGGL(k_gbt_exact_partition, dim3(gR, (unsigned)A), dim3(256), 0, s, bBf.as<float>(), bPos.as<uint8_t>(), rt.S, rt.F, rt.B, d, G);
    }
    for (int d = 0; !exact && d < D; ++d) {
      const int nl = 1 << d, fg = (G.F + fpb[d] - 1) / fpb[d];
      long long* Hcur = bLev.as<long long>() + (size_t)(d & 1) * lev_entries;
      const long long* Hprev = bLev.as<long long>() + (size_t)((d & 1) ^ 1) * lev_entries;
      hipLaunchKernelGGL(k_gbt_hist, dim3((unsigned)fg, (unsigned)A, (unsigned)nsl[d]), dim3(HIST_T), (size_t)fpb[d] * nl * 512 * 8, s, bBq.as<uint8_t>(),
                         bG.as<long long>(), bH.as<long long>(), bPos.as<uint8_t>(), rt.S, dBuild, bPart.as<long long>(), d, fpb[d], nsl[d], G);
      hipLaunchKernelGGL(k_gbt_split, dim3((unsigned)nl, (unsigned)A, SPLIT_CHUNKS), dim3(256), 0, s, bPart.as<long long>(), bNcut.as<int32_t>(), rt.G,
                         rt.H, rt.S, dBuild, Hprev, Hcur, bCand.as<Best>(), d, nsl[d], P.lambda, P.gamma, P.min_child_weight, G);
      hipLaunchKernelGGL(k_gbt_split_pick, dim3((unsigned)((A * nl + 63) / 64)), dim3(64), 0, s, bCand.as<Best>(), rt, d, A);
      hipLaunchKernelGGL(k_gbt_partition, dim3(gR, (unsigned)A), dim3(256), 0, s, bBq.as<uint8_t>(), bPos.as<uint8_t>(), rt.S, rt.F, rt.B, dCnt, d, G);
      if (d + 1 < D) hipLaunchKernelGGL(k_gbt_choose, dim3((unsigned)((A * nl + 63) / 64)), dim3(64), 0, s, rt.S, dCnt, dBuild, d, A);
    }
    hipLaunchKernelGGL(k_gbt_close, dim3((unsigned)((A * GBT_MAXN + 255) / 256)), dim3(256), 0, s, rt, A, P.eta, P.lambda);
    hipLaunchKernelGGL(k_gbt_margin, dim3(gRA), dim3(256), 0, s, bFm.as<float>(), bPos.as<uint8_t>(), rt.V, G);
    GNX_HIPRET(hipGetLastError());
  }
  const GbtTables unread = tab.at(tab_n);  // the loss after the last round: the same pass, its root sums where no tree is
  grad(P.n_rounds, unread.G, unread.H, unread.S);
  GNX_HIPRET(hipGetLastError());

  // ---- trees back to the host, nodes in heap order ----
  GbtHostTables h;
  std::vector<long long> hL((size_t)P.n_rounds + 1);
  GNX_HIPRET(h.fetch(tab, tab_n, s));
  GNX_HIPRET(hipMemcpyAsync(hL.data(), bLoss.p, hL.size() * 8, hipMemcpyDeviceToHost, s));
  GNX_HIPRET(hipStreamSynchronize(s));
  *n_nodes_out = gbt_compact_trees(
      h.S, T, tree_off, left, right,
      [&](int64_t q, size_t i) {
        feat[q] = h.F[i];
        if (exact) std::memcpy(&cond[q], &h.B[i], 4);   // the threshold's float32 bits
        else cond[q] = cuts[(size_t)(h.F[i] % A) * 256 + h.B[i]];
      },
      [&](int64_t q, size_t i) { feat[q] = 0; cond[q] = h.V[i]; });
  for (int t = 0; t < T; ++t) tree_class[t] = t % A;
  if (loss_out)
    for (int r = 0; r <= P.n_rounds; ++r) loss_out[r] = ((double)hL[(size_t)r] / 16777216.0) / (double)G.R;
  return hipSuccess;
}

