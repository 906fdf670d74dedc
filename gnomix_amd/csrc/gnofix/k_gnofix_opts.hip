// k_gnofix_opts.hip — the Gnofix re-phasing loop with the reference's search options (gfx950).
//
// gnofix() of the reference (src/Gnofix/gnofix.py:58-208) with check_criterion, max_center_offset, non_lin_s, prob_comp,
// prior_switch_prob and padding as arguments.  k_gnofix.hip is the same loop with all six at their defaults and is what the default
// values still run (gnx_api.hip dispatches); this kernel is reached by every other setting.  It keeps k_gnofix's data: the u16 rank
// strips (read-only), the per-row cache of largest probabilities from the initial smoother pass, k_gnofix_dif before and
// k_gnofix_swap after, and leaf sums in tree order in float32.  It leaves out k_gnofix's lazy re-evaluation and its memory of
// rejected candidates: both are arguments about the default candidate (one single switch at w) and do not carry over.
//
// What the options change, each as the reference BEHAVES:
//  * Candidates of a checked window w inside the centers: single switches at j = w-off .. w+off, double switches [w-j, w) for
//    j = 1 .. non_lin_s-1 and [w, w+j+1) for j = 0 .. non_lin_s-1, in that order (gnofix.py:133-136); outside the centers off and
//    non_lin_s are 0 and the scope is clipped (gnofix.py:122-127).  All 2K switched rows of a window are ONE batch of walks: a row is
//    the scope tile of the two logical strips plus "read the other haplotype at positions [f1, f2)", so no row is ever materialised.
//  * The two original rows are what the smoother's row center + 1 sees: their probabilities come from the cache.
//  * np.argmax over the candidates: the first maximum wins.  prob_comp "max": the larger of the two haplotypes' largest
//    probabilities; "prod": their float32 product (gnofix.py:160-163).
//  * Acceptance (gnofix.py:171): best * prior > orig * (1 - prior) with both products in FLOAT32.  This is numpy >= 2 (NEP 50): a
//    Python float next to a float32 scalar is "weak" and the product stays float32; 1 - prior is a Python-float (double) subtraction
//    first, then each factor is rounded to float32.
//  * An accepted double switch [j1, j2) exchanges B and the tracker on [j1, j2), but M_track is rebuilt from zeros for each index
//    (gnofix.py:184-189) and only the LAST one reaches correct_phase_error: X is exchanged from j2 on.  Hence two parities: parB
//    (strips, labels, cache, "disc_base") and parX (convergence signature, final SNP swap).
//  * A single switch at j = 0 (w = off = (S-1)/2) exchanges all of B; M_track is constant and X stays as it is.
//  * "disc_base" compares the first-maximum argmax of the float64 B at w-1 and w under the CURRENT parB (k_gnofix_argmax computes
//    the physical argmax once); "disc_either" is that OR "disc_smooth"; "all" checks every window of the iteration set.
//  * padding = 0 walks the centers only (gnofix.py:84).
// After an accepted switch on [j1, j2): smoother rows that see only exchanged windows exchange their two labels and cache entries,
// rows that see windows on both sides of j1 or j2 are re-evaluated at once, the others keep what they have.
//
// A calibrated model (Smoother.calibrate with a fitted Calibrator) runs this kernel for EVERY option set, the defaults included:
// smoother.predict (gnofix.py:80,190) goes through Smoother.predict_proba and is argmax(Calibrator.transform(raw)), so every label of
// a smoother row — the initial ones (Y0, from a labels-only k_calibrate launch) and the re-evaluated ones — is the calibrated label
// of gnx_calibrate.h.  smoother.model.predict_proba (gnofix.py:157) is the raw model: the cache of largest probabilities, prob_comp
// and the acceptance test stay on the raw float32 softmax.  The maps are read from global memory (a few KB, L2-resident).
//
// One 256-thread workgroup per individual; every decision is block-uniform (taken from LDS after a barrier).
#include "../gnx_internal.h"
#include "../gnx_rank.h"
#include "../gnx_exp.h"
#include "../gnx_calibrate.h"

namespace {

constexpr int OT = 256;  // threads per individual

struct GnofixOptsLds {
  size_t seg, Y, pmax, am, parB, parX, dif, dirty, desc, rmax, rlab, leaf, marg, ct0, total;
  int rows_cap, rc;
};

__host__ __device__ inline int gnofix_opts_rows_cap(int S) { return 4 * S > 2 * (S + 2) ? 4 * S : 2 * (S + 2); }

// rc = rows evaluated side by side: their leaves [rc][n_trees] and margins [rc][A] share 48 KB
__host__ __device__ inline GnofixOptsLds gnofix_opts_lds(int W, int A, int S, int GP, int n_trees) {
  auto r16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t NWD = (size_t)(W + 31) / 32;
  GnofixOptsLds o{};
  o.rows_cap = gnofix_opts_rows_cap(S);
  const size_t per_row = ((size_t)n_trees + A) * 4;
  size_t rc = (size_t)49152 / per_row;
  if (rc > (size_t)o.rows_cap) rc = (size_t)o.rows_cap;
  o.rc = (int)rc;
  size_t off = 0;
  o.seg = off; off += r16((size_t)2 * A * GP * 2);
  o.Y = off; off += r16((size_t)W * 2);
  o.pmax = off; off += r16((size_t)2 * W * 4);
  o.am = off; off += r16((size_t)W * 2);
  o.parB = off; off += r16(NWD * 4);
  o.parX = off; off += r16(NWD * 4);
  o.dif = off; off += r16(NWD * 4);
  o.dirty = off; off += r16(NWD * 4);
  o.desc = off; off += r16((size_t)o.rows_cap * 8);
  o.rmax = off; off += r16((size_t)o.rows_cap * 4);
  o.rlab = off; off += r16((size_t)o.rows_cap);
  o.leaf = off; off += r16(rc * n_trees * 4);
  o.marg = off; off += r16(rc * A * 4);
  o.ct0 = off; off += r16((size_t)(A + 1) * 4);
  o.total = off;
  return o;
}

struct GnofixOptsK {
  const uint16_t* R;
  const uint32_t* dif;
  uint32_t* par;          // out: final X parity
  const uint32_t* gf;
  const int32_t* class_tree0;
  const int32_t* Y0;
  const float* P0;
  const uint8_t* am;      // [2n][W] first-maximum argmax of the float64 B
  int32_t* Yout;
  int32_t* n_switches;
  uint32_t* hist;
  int32_t W, A, S, max_it, D, NT, GP;
  int32_t criterion, off, nls, prod, padding;
  float base_score, prior, one_minus_prior;
  CalibMaps cal;          // cal.off != NULL: smoother rows carry calibrated labels
};

// ---- pre-pass: np.argmax(B, axis=-1) on the float64 base probabilities (first maximum; a NaN counts as the maximum) ----
__global__ __launch_bounds__(256) void k_gnofix_argmax(const double* __restrict__ B, int64_t rows, int A, uint8_t* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double* p = B + r * A;
  int best = 0;
  double bv = p[0];
  for (int a = 1; a < A; ++a) {
    const double v = p[a];
    if (bv == bv && (v > bv || v != v)) { bv = v; best = a; }
  }
  out[r] = (uint8_t)best;
}

__device__ __forceinline__ void flip_range(uint32_t* par, int NWD, int lo, int hi, int tid) {  // windows [lo, hi)
  for (int q = tid; q < NWD; q += OT) {
    const int b0 = q * 32;
    if (b0 + 32 > lo && b0 < hi) {
      uint32_t m = 0xffffffffu;
      if (lo > b0) m &= 0xffffffffu << (lo - b0);
      if (hi < b0 + 32) m &= 0xffffffffu >> (b0 + 32 - hi);
      par[q] ^= m;
    }
  }
}

__global__ __launch_bounds__(OT) void k_gnofix_opts(GnofixOptsK L) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int W = L.W, A = L.A, S = L.S, pad = (S + 1) / 2, half = (S - 1) / 2;
  const int D = L.D, NWD = (W + 31) / 32, GP = L.GP, TW = gnx_gf_tree_words(D), NT = L.NT;
  const int tid = threadIdx.x, ln = tid & 63;
  const int64_t ind = blockIdx.x;
  const GnofixOptsLds o = gnofix_opts_lds(W, A, S, GP, NT);
  uint16_t* seg = reinterpret_cast<uint16_t*>(lds + o.seg);     // [2][A][GP] ranks of the two logical strips around the work
  uint16_t* Y = reinterpret_cast<uint16_t*>(lds + o.Y);         // labels: maternal | paternal << 8
  float* pmax = reinterpret_cast<float*>(lds + o.pmax);         // [W][2] largest probability of (window, haplotype)'s smoother row
  uint16_t* am = reinterpret_cast<uint16_t*>(lds + o.am);       // argmax of B: physical haplotype 0 | haplotype 1 << 8
  uint32_t* parB = reinterpret_cast<uint32_t*>(lds + o.parB);   // logical haplotype h at window u = physical h ^ parB(u)
  uint32_t* parX = reinterpret_cast<uint32_t*>(lds + o.parX);   // the same for the SNP blocks
  uint32_t* dif = reinterpret_cast<uint32_t*>(lds + o.dif);
  uint32_t* dirty = reinterpret_cast<uint32_t*>(lds + o.dirty); // smoother rows to re-evaluate
  uint32_t* desc = reinterpret_cast<uint32_t*>(lds + o.desc);   // per row: {haplotype | tile shift << 1, f1 | f2 << 16}
  float* rmax = reinterpret_cast<float*>(lds + o.rmax);         // per row: largest probability
  uint8_t* rlab = lds + o.rlab;                                 // per row: its first arg-max
  float* leaf = reinterpret_cast<float*>(lds + o.leaf);         // [rc][NT]
  float* marg = reinterpret_cast<float*>(lds + o.marg);         // [rc][A]
  int* ct0s = reinterpret_cast<int*>(lds + o.ct0);
  uint32_t* hist = L.hist + (size_t)ind * (L.max_it > 0 ? L.max_it : 1) * NWD;
  const uint16_t* __restrict__ R0 = L.R + (size_t)2 * ind * W * A;
  const uint32_t* __restrict__ GT = L.gf;
  const size_t WA = (size_t)W * A;
  const uint32_t invA = 0xFFFFFFFFu / (uint32_t)A + 1u;    // n / A  = umulhi(n, invA)  for n < 65536
  const uint32_t invP = 0xFFFFFFFFu / (uint32_t)GP + 1u;   // n / GP = umulhi(n, invP)  for n < 65536
  const int RC = o.rc;

  for (int u = tid; u < W; u += OT) {
    Y[u] = (uint16_t)(L.Y0[(size_t)2 * ind * W + u] | (L.Y0[(size_t)(2 * ind + 1) * W + u] << 8));
    pmax[2 * u] = L.P0[(size_t)2 * ind * W + u];
    pmax[2 * u + 1] = L.P0[(size_t)(2 * ind + 1) * W + u];
    am[u] = (uint16_t)(L.am[(size_t)2 * ind * W + u] | ((uint16_t)L.am[(size_t)(2 * ind + 1) * W + u] << 8));
  }
  for (int q = tid; q < NWD; q += OT) { parB[q] = 0; parX[q] = 0; dirty[q] = 0; dif[q] = L.dif[(size_t)ind * NWD + q]; }
  if (tid <= A) ct0s[tid] = L.class_tree0[tid];
  __syncthreads();

  auto pbit = [&](int u) -> int { return (int)((parB[u >> 5] >> (u & 31)) & 1u); };
  // check() of gnofix.py:25-45 at window w >= 1, from the current labels / the current logical B
  auto checked = [&](int w) -> bool {
    if (L.criterion == GNX_GNOFIX_CHECK_ALL) return true;
    bool c = false;
    if (L.criterion != GNX_GNOFIX_CHECK_DISC_BASE) c = Y[w] != Y[w - 1];
    if (L.criterion != GNX_GNOFIX_CHECK_DISC_SMOOTH) {
      // {argmax of logical m, argmax of logical p}: the two bytes in physical order, exchanged where parB is odd — as a PAIR
      // comparison "m differs or p differs" needs the bytes in logical order
      uint16_t a1 = am[w], a0 = am[w - 1];
      if (pbit(w)) a1 = (uint16_t)((a1 >> 8) | (a1 << 8));
      if (pbit(w - 1)) a0 = (uint16_t)((a0 >> 8) | (a0 << 8));
      c = c || a1 != a0;
    }
    return c;
  };
  // first checked window in [from, end): every wave for itself, lane = window (the state it reads is stable between barriers)
  auto next_checked = [&](int from, int end) -> int {
    for (int w0 = from; w0 < end; w0 += 64) {
      const int w = w0 + ln;
      const bool c = w < end && checked(w);
      const unsigned long long bal = __ballot(c);
      if (bal) return w0 + __builtin_ctzll(bal);
    }
    return end;
  };
  auto first_dirty = [&]() -> int {
    for (int q0 = 0; q0 < NWD; q0 += 64) {
      const int q = q0 + ln;
      const uint32_t m = q < NWD ? dirty[q] : 0u;
      const unsigned long long bal = __ballot(m != 0);
      if (bal) {
        const int first = __builtin_ctzll(bal);
        const uint32_t mw = (uint32_t)__shfl((int)m, first);
        return min(W, (q0 + first) * 32 + __builtin_ctz(mw));
      }
    }
    return W;
  };

  // The smoother on rows desc[0 .. nrows) of the tile: rmax / rlab.  Row = haplotype h of the tile, shifted by `shift` positions,
  // reading the OTHER haplotype at tile positions [f1, f2).  RC rows at a time: lane = (tree, row) walks one tree on one row and
  // parks the leaf; one lane per (row, class) adds the class's leaves in tree order (float32: bit-identical to the sequential
  // predictor); one lane per row takes xgboost's Softmax.  want_lab: the rows' labels are used (re-evaluated smoother rows; the
  // candidates of a window are compared by probability only) — a calibrated model then pays the maps for those rows alone.
  // Called by all threads; ends with a barrier.
  const bool calibrated = L.cal.off != nullptr;
  auto eval_rows = [&](int nrows, bool want_lab) {
    for (int c0 = 0; c0 < nrows; c0 += RC) {
      const int nr = min(RC, nrows - c0);
      const uint32_t invN = nr > 1 ? 0xFFFFFFFFu / (uint32_t)nr + 1u : 0u;  // e / nr = umulhi(e, invN): nr * NT <= 12288 < 65536 (the 48 KB of leaves).
      // invN = 0 is a SENTINEL for nr = 1: 2^32 / 1 does not fit 32 bits, and e / 1 = e needs no multiply (tested below)
      for (int e = tid; e < nr * NT; e += OT) {
        const int t = invN ? (int)__umulhi((uint32_t)e, invN) : e, r = e - t * nr;
        const uint32_t d0 = desc[2 * (c0 + r)], d1 = desc[2 * (c0 + r) + 1];
        const uint32_t h = d0 & 1u, shift = d0 >> 1, f1 = d1 & 0xffffu, f2 = d1 >> 16;
        const uint32_t tb = (uint32_t)t * (uint32_t)TW;
        uint32_t j = 1;
        for (int d = 0; d < D; ++d) {
          const uint32_t nd = GT[tb + j];
          const uint32_t off2 = (nd & 0xffffu) >> 1;                 // a * GP + s
          const uint32_t s = off2 - __umulhi(off2, invP) * (uint32_t)GP;
          const uint32_t hh = h ^ ((s >= f1 && s < f2) ? 1u : 0u);
          const uint32_t rk = seg[hh * (uint32_t)(A * GP) + off2 + shift];
          j = 2 * j + (((nd >> 16) <= rk) ? 1u : 0u);
        }
        leaf[r * NT + t] = __uint_as_float(GT[tb + j]);
      }
      __syncthreads();
      for (int e = tid; e < nr * A; e += OT) {
        const int r = (int)__umulhi((uint32_t)e, invA), c = e - r * A;
        const float* lb = leaf + r * NT;
        float ps = 0.f;
        for (int t = ct0s[c]; t < ct0s[c + 1]; ++t) ps += lb[t];
        marg[e] = L.base_score + ps;
      }
      __syncthreads();
      for (int r = tid; r < nr; r += OT) {
        float* mr = marg + r * A;
        float wmax = mr[0];
        for (int a = 1; a < A; ++a) wmax = fmaxf(mr[a], wmax);
        double wsum = 0.0;
        for (int a = 0; a < A; ++a) { const float ex = gnx_softmax_exp(mr[a] - wmax); mr[a] = ex; wsum += (double)ex; }
        const float fs = (float)wsum;
        int best = 0;
        float bv = mr[0] / fs;
        for (int a = 1; a < A; ++a) { const float v = mr[a] / fs; if (v > bv) { bv = v; best = a; } }
        rmax[c0 + r] = bv;   // raw, calibrated or not
        if (calibrated && want_lab)   // the float32 quotients are what the batched smoother stores and k_calibrate reads
          best = gnx_calib_row(L.cal, A, [&](int c) -> double { return (double)(mr[c] / fs); }, [](int, double) {});
        rlab[c0 + r] = (uint8_t)best;
      }
      __syncthreads();
    }
  };

  const int w_begin = L.padding ? 1 : half, w_end = L.padding ? W : W - half;  // gnofix.py:83-84
  int n_switch = 0;
  for (int it = 0; it < L.max_it; ++it) {
    // ---- convergence: has this X_m been seen at the start of an earlier sweep? (gnofix.py:108-113) ----
    int seen = 0;
    for (int k = tid; k < it; k += OT) {
      bool same = true;
      for (int q = 0; q < NWD; ++q) same = same && hist[(size_t)k * NWD + q] == (parX[q] & dif[q]);
      seen |= same ? 1 : 0;
    }
    if (__syncthreads_or(seen)) break;
    for (int q = tid; q < NWD; q += OT) hist[(size_t)it * NWD + q] = parX[q] & dif[q];

    int from = w_begin;
    while (true) {
      const int w = __builtin_amdgcn_readfirstlane(next_checked(from, w_end));
      if (w >= w_end) break;
      from = w + 1;
      const bool inside = w >= half && w <= W - 1 - half;                 // "w in centers"
      const int center = min(max(w, half), W - 1 - half), lo = center - half;
      const int off_w = inside ? L.off : 0, nls_w = inside ? L.nls : 0;
      const int n_single = 2 * off_w + 1, n_left = max(nls_w - 1, 0), K = n_single + n_left + nls_w;
      auto cand = [&](int k, int& j1, int& j2) {   // exchanged windows [j1, j2); j2 = W: a single switch
        if (k < n_single) { j1 = w - off_w + k; j2 = W; }
        else if (k < n_single + n_left) { j1 = w - (k - n_single + 1); j2 = w; }
        else { j1 = w; j2 = w + (k - n_single - n_left) + 1; }
      };
      // the scope [lo, lo + S) of both logical strips
      for (int e = tid; e < 2 * S * A; e += OT) {
        const int h = e >= S * A ? 1 : 0, f = e - h * S * A;
        const int s = (int)__umulhi((uint32_t)f, invA), a = f - s * A;
        const int u = lo + s;
        seg[(h * A + a) * GP + s] = R0[(size_t)(h ^ pbit(u)) * WA + (size_t)u * A + a];
      }
      for (int r = tid; r < 2 * K; r += OT) {
        int j1, j2;
        cand(r >> 1, j1, j2);
        const uint32_t f1 = (uint32_t)max(j1 - lo, 0), f2 = (uint32_t)min(j2 - lo, S);
        desc[2 * r] = (uint32_t)(r & 1);
        desc[2 * r + 1] = f1 | (f2 << 16);
      }
      __syncthreads();
      eval_rows(2 * K, false);
      // np.argmax over the candidates, then gnofix.py:171 in float32
      float best = 0.f;
      int kb = 0;
      for (int k = 0; k < K; ++k) {
        const float a = rmax[2 * k], b = rmax[2 * k + 1];
        const float p = L.prod ? a * b : fmaxf(a, b);
        if (k == 0 || p > best) { best = p; kb = k; }
      }
      const float oa = pmax[2 * (center + 1)], ob = pmax[2 * (center + 1) + 1];
      const float orig = L.prod ? oa * ob : fmaxf(oa, ob);
      const bool accept = best * L.prior > orig * L.one_minus_prior;
      if (!accept) continue;  // (two barriers lie between this read of rmax and the next batch's write)

      ++n_switch;
      int j1, j2;
      cand(kb, j1, j2);
      const int jl = j2 < W ? j2 : j1;  // the index correct_phase_error sees: the last one of best_switch
      __syncthreads();
      flip_range(parB, NWD, j1, j2, tid);
      if (jl >= 1) flip_range(parX, NWD, jl, W, tid);
      // smoother row wr sees the windows [mn, mx] (reflect padding included)
      for (int wr = tid; wr < W; wr += OT) {
        int mn = W, mx = -1;
        const int p0 = wr, p1 = wr + S - 1;
        const int a0 = max(p0, pad), a1 = min(p1, pad + W - 1);
        if (a0 <= a1) { mn = min(mn, a0 - pad); mx = max(mx, a1 - pad); }
        if (p0 < pad) { const int b1 = min(p1, pad - 1); mn = min(mn, pad - 1 - b1); mx = max(mx, pad - 1 - p0); }
        if (p1 >= pad + W) { const int b0 = max(p0, pad + W); mn = min(mn, W - 1 - (p1 - pad - W)); mx = max(mx, W - 1 - (b0 - pad - W)); }
        if (mn >= j1 && mx < j2) {
          const uint16_t y = Y[wr];
          Y[wr] = (uint16_t)((y >> 8) | (y << 8));
          const float t0 = pmax[2 * wr];
          pmax[2 * wr] = pmax[2 * wr + 1];
          pmax[2 * wr + 1] = t0;
        } else if (mx >= j1 && mn < j2) {
          atomicOr(&dirty[wr >> 5], 1u << (wr & 31));
        }
      }
      __syncthreads();
      // ---- re-evaluate the marked rows, up to S + 2 consecutive windows x 2 haplotypes per tile ----
      while (true) {
        const int gb = __builtin_amdgcn_readfirstlane(first_dirty());
        if (gb >= W) break;
        const int nwin = min(S + 2, W - gb), nj = nwin + S - 1;
        __syncthreads();  // (every wave has read the mask)
        for (int e = tid; e < 2 * nj * A; e += OT) {
          const int h = e >= nj * A ? 1 : 0, f = e - h * nj * A;
          const int q = (int)__umulhi((uint32_t)f, invA), a = f - q * A;
          const int u = gnx_slide_src(gb + q, W, pad);
          seg[(h * A + a) * GP + q] = R0[(size_t)(h ^ pbit(u)) * WA + (size_t)u * A + a];
        }
        for (int r = tid; r < 2 * nwin; r += OT) {
          const int h = r >= nwin ? 1 : 0, rk = r - h * nwin;
          desc[2 * r] = (uint32_t)h | ((uint32_t)rk << 1);
          desc[2 * r + 1] = 0u;
        }
        for (int q = tid; q < NWD; q += OT) {
          const int b0 = q * 32;
          if (b0 + 32 > gb && b0 < gb + nwin) {
            uint32_t m = 0xffffffffu;
            if (gb > b0) m &= 0xffffffffu << (gb - b0);
            if (gb + nwin < b0 + 32) m &= 0xffffffffu >> (b0 + 32 - gb - nwin);
            dirty[q] &= ~m;
          }
        }
        __syncthreads();
        eval_rows(2 * nwin, true);
        for (int r = tid; r < 2 * nwin; r += OT) {
          const int h = r >= nwin ? 1 : 0, rk = r - h * nwin;
          reinterpret_cast<uint8_t*>(Y)[2 * (gb + rk) + h] = rlab[r];
          pmax[2 * (gb + rk) + h] = rmax[r];
        }
        __syncthreads();
      }
    }
    __syncthreads();  // (this sweep's history row is complete before the next convergence test reads it)
  }

  __syncthreads();
  for (int u = tid; u < W; u += OT) {
    L.Yout[(size_t)2 * ind * W + u] = Y[u] & 0xff;
    L.Yout[(size_t)(2 * ind + 1) * W + u] = Y[u] >> 8;
  }
  for (int q = tid; q < NWD; q += OT) L.par[(size_t)ind * NWD + q] = parX[q];
  if (tid == 0 && L.n_switches) L.n_switches[ind] = n_switch;
}

}  // namespace

size_t gnx_gnofix_opts_lds_bytes(int W, int A, int S, int pitch, int n_trees, int* rows_side_by_side) {
  const GnofixOptsLds o = gnofix_opts_lds(W, A, S, pitch, n_trees);
  if (rows_side_by_side) *rows_side_by_side = o.rc;
  return o.total;
}

// after the initial smoother pass (Y0, proba0) and gnx_launch_gnofix_prep; am: [2 n_ind][W] bytes of scratch
// cal: the maps of a calibrated model (Y0 then holds calibrated labels, proba0 the RAW probabilities), or NULL
hipError_t gnx_launch_gnofix_opts(const GnofixLaunch& G, int64_t n_ind, const gnx_gnofix_opts& O, uint8_t* am, const CalibMaps* cal,
                                  hipStream_t s) {
  if (n_ind <= 0) return hipSuccess;
  int rc = 0;
  const size_t lds = gnx_gnofix_opts_lds_bytes(G.W, G.A, G.S, G.gf_pitch, G.d.n_trees, &rc);
  if (lds > (size_t)160 * 1024 || rc < 1) return hipErrorInvalidValue;
  hipError_t e = gnx_launch_gnofix_pmax(G, n_ind, s);
  if (e != hipSuccess) return e;
  const int64_t rows = 2 * n_ind * (int64_t)G.W;
  hipLaunchKernelGGL(k_gnofix_argmax, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, G.B, rows, G.A, am);
  const float prior = (float)O.prior_switch_prob, omp = (float)(1.0 - O.prior_switch_prob);
  const GnofixOptsK L{G.R, G.dif, G.par, G.gf, G.class_tree0, G.Y0, G.pmax0, am, G.Yout, G.n_switches, G.hist, G.W, G.A, G.S, G.max_it,
                      G.d.D, G.d.n_trees, G.gf_pitch, O.check_criterion, O.max_center_offset, O.non_lin_s,
                      O.prob_comp == GNX_GNOFIX_PROB_PROD ? 1 : 0, O.padding ? 1 : 0, G.d.base_score, prior, omp,
                      cal ? *cal : CalibMaps{nullptr, nullptr, nullptr, 0}};
  GNX_LDS_OPTIN(lds, k_gnofix_opts);
  hipLaunchKernelGGL(k_gnofix_opts, dim3((unsigned)n_ind), dim3(OT), lds, s, L);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return gnx_launch_gnofix_swap(G, n_ind, s);
}
