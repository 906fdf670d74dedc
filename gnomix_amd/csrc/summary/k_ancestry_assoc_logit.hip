// summary/k_ancestry_assoc_logit.hip — the ancestry-specific association for case / control traits: one logistic fit per SNP (the Tractor
// model with a logit link), iterated ON THE DEVICE.  include/gnomix_hip.h states the model, the iteration rule and the outputs;
// DESIGN.md section 4.19 the layout, the summation order and the cost model.
//
// k_ancestry_assoc_logit_prep: one thread per individual: part[i], zy[i] = (Z[i, :K], y[i]) and the count of phenotypes that are
//   neither 0 nor 1 among the individuals with use != 0 and a finite y.
// k_ancestry_assoc_logit_null: ONE workgroup per window of the range: n, n_case, sum_h, the labels out of range among ALL rows, and the
//   fit of the null model U = [Z, kept h] from theta = 0 (P = K + A - 1 columns).
// k_ancestry_assoc_logit_snp<KIND>: ONE wave per tile of TC adjacent SNPs, lane = SNP, tiles cut at window boundaries (so labels,
//   participation and covariates are the same in every lane and only the genotype code differs); the wave walks ALL individuals once
//   per evaluation of (deviance, g, H).  The fit of every lane is a small state machine (evaluate -> factor -> step / halve -> ... ->
//   final evaluation); a lane that is done idles until the tile's last lane is.
// Both fits are one function, lg_fit<KIND, NULLFIT>: the null kernel runs it in lane 0 with no dosage columns.
//
// A lane's state lives in its own column of LDS, [slot][TC lanes] float64 (conflict-free: adjacent lanes, adjacent words): theta, the
// candidate theta, the step, g, the scale and H as a packed lower triangle (row j, column k <= j at j (j + 1) / 2 + k), which the
// Cholesky factor overwrites.  NS = 5 q + q (q + 1) / 2 slots for q columns; TC = min(64, 80 KiB / (8 NS)), two workgroups per CU.
// No per-thread array, no scratch.
//
// SUMMATION ORDER.  Every float64 sum over individuals (the deviance, g, H) runs over the individuals in ascending i, one term per
// individual, each product rounded once (no fused multiply-add outside gnx_exp.h's exp), added to the running sum; individuals that
// take no part and terms whose column value is zero are skipped, which leaves the sum unchanged.  eta adds x_j theta_j in ascending
// column j.  An H term is (w x_j) x_k for j >= k, a g term r x_j.  The order is a function of N alone: a SNP's results depend on its
// column, its window's labels, y, Z, use and the scalar arguments only (not on [c0, c1), TC, the grid or the row form).
//
// This is the VALU form.  The dense block H_UU = sum_i w_i u_i u_i^T of a tile is a float64 product (tile x n) (n x P (P + 1) / 2) that
// v_mfma_f64_16x16x4 could carry; it is NOT built here (DESIGN.md section 4.19 says what that would take).
#include "../gnx_exp.h"
#include "gnx_summary_host.h"

namespace {

constexpr int LG_THREADS = 64;
constexpr size_t LG_LDS_BYTES = 80 * 1024;     // two workgroups per CU (160 KiB)
constexpr double LG_PIVOT_MIN = 0x1p-40;       // the host rule of gnomix_amd/assoc.py
constexpr double LG_W_MIN = 0x1p-40;
constexpr int LG_MAX_HALVINGS = 10;

// the blocks' sizes: the only definition of the layout (the header states it)
struct LgLayout {
  int P, Q, SF, SI, WF, WI;
  __host__ __device__ LgLayout(int A, int K) {
    P = K + A - 1;
    Q = K + 2 * A - 1;
    SF = 2 * A + 1;      // beta (A), se (A), dev
    SI = 2 * A + 3;      // n_alt (A), n_alt_case (A), n_miss, iters, status
    WF = P + 1;          // theta0 (P), dev0
    WI = A + 4;          // n, n_case, sum_h (A), iters0, status0
  }
};
__host__ __device__ inline int lg_slots(int q) { return 5 * q + q * (q + 1) / 2; }

__global__ __launch_bounds__(256) void k_ancestry_assoc_logit_prep(const double* __restrict__ y, const double* __restrict__ Z,
                                                                   const uint8_t* __restrict__ use, int64_t n_ind, int K, double* __restrict__ zy,
                                                                   uint8_t* __restrict__ part, unsigned long long* __restrict__ bad_y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ind) return;
  const int K1 = K + 1;
  const double yi = y[i];
  bool ok = (use == nullptr || use[i] != 0) && isfinite(yi);
  if (ok && yi != 0.0 && yi != 1.0) atomicAdd(bad_y, 1ull);
  for (int k = 0; k < K; ++k) {
    const double z = Z[i * K + k];
    ok = ok && isfinite(z);
    zy[i * K1 + k] = z;
  }
  zy[i * K1 + K] = yi;
  part[i] = ok ? 1 : 0;
}

enum { LG_INIT = 0, LG_NEWTON = 1, LG_LINE = 2, LG_FINAL = 3, LG_DONE = 4 };

// One fit per lane.  NULLFIT: the window's null model (nq = P columns; of / oi = the window's rows of win_f64 / win_i32; the labels out
// of range among all rows are added to *bad).  Else the SNP's full model (nq = Q columns; wf / wi = its window's null results).
template <int KIND, bool NULLFIT>
__device__ __forceinline__ void lg_fit(double* __restrict__ lds, const int TC, const int lane, const bool active, const uint8_t* __restrict__ rows,
                                       const int64_t ld, const int32_t* __restrict__ lw, const int64_t ldl, const int64_t n_ind, const int A,
                                       const int K, const int64_t c, const double* __restrict__ zy, const uint8_t* __restrict__ part,
                                       const int min_ac, const double tol, const int max_iter, const double* __restrict__ wf,
                                       const int32_t* __restrict__ wi, double* __restrict__ of, int32_t* __restrict__ oi, double* __restrict__ oth,
                                       unsigned long long* __restrict__ bad) {
  const LgLayout L(A, K);
  const int K1 = K + 1, P = L.P, Am1 = A - 1;
  const int nq = NULLFIT ? L.P : L.Q;
  const int oTH = 0, oTE = nq, oDL = 2 * nq, oG = 3 * nq, oS = 4 * nq, oH = 5 * nq, NS = lg_slots(nq);
#define LG(slot) lds[(size_t)(slot) * TC + lane]
  // int32 scratch of the counting pass: entry e in one half of the lane's own float64 slot e / 2
  int32_t* li = reinterpret_cast<int32_t*>(lds);
#define LGI(e) li[((size_t)((e) >> 1) * TC + lane) * 2 + ((e) & 1)]
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int state = active ? LG_INIT : LG_DONE;
  int status = 0, it = 0, halv = 0;
  uint32_t keep = 0;         // the dosage columns the column rule keeps
  double dev_cur = 0.0, tstep = 1.0;

  if (active) {
    // ---- the integers (exact) --------------------------------------------------------------------------------------------------------
    const int ne = NULLFIT ? A + 2 : 2 * A + 1;   // null: n, n_case, sum_h[A]; SNP: n_alt[A], n_alt_case[A], n_miss
    for (int e = 0; e < ne; ++e) LGI(e) = 0;
    unsigned long long nbad = 0;
    for (int64_t i = 0; i < n_ind; ++i) {
      const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
      const bool oa = la >= 0 && la < A, ob = lb >= 0 && lb < A;
      if (NULLFIT) nbad += (oa ? 0 : 1) + (ob ? 0 : 1);
      if (!part[i] || !oa || !ob) continue;
      const int yc = zy[i * K1 + K] == 1.0;
      if (NULLFIT) {
        LGI(0) += 1;
        LGI(1) += yc;
        LGI(2 + la) += 1;
        LGI(2 + lb) += 1;
      } else {
        const uint32_t ca = as_code<KIND>(rows + (2 * i) * ld, c), cb = as_code<KIND>(rows + (2 * i + 1) * ld, c);
        LGI(2 * A) += (ca > 1u) + (cb > 1u);
        if (ca == 1u) { LGI(la) += 1; LGI(A + la) += yc; }
        if (cb == 1u) { LGI(lb) += 1; LGI(A + lb) += yc; }
      }
    }
    if (NULLFIT && nbad) atomicAdd(bad, nbad);
    int n, p_kept = K;
    if (NULLFIT) {
      n = LGI(0);
      for (int e = 0; e < ne; ++e) oi[e] = LGI(e);
      for (int a = 0; a < Am1; ++a) p_kept += LGI(2 + a) > 0;
    } else {
      n = wi[0];
      for (int a = 0; a < Am1; ++a) p_kept += wi[2 + a] > 0;
      for (int a = 0; a < A; ++a) {
        const int na = LGI(a), nc = LGI(A + a);
        if (na >= min_ac && nc > 0 && nc < na) { keep |= 1u << a; ++p_kept; }
      }
      for (int e = 0; e < ne; ++e) oi[e] = LGI(e);
      if (wi[3 + A] != 0) status = 4;
    }
    if (status == 0 && n - p_kept < 1) status = 2;
    if (status != 0) state = LG_DONE;
    // ---- the start: theta = 0 (null), or the window's null theta with beta = 0 ---------------------------------------------------------
    for (int e = 0; e < NS; ++e) LG(e) = 0.0;
    if (!NULLFIT && status == 0)
      for (int j = 0; j < P; ++j) { LG(oTH + j) = wf[j]; LG(oTE + j) = wf[j]; }
  }

  double dev_e = 0.0, wmin = 0.0;
  while (__any(state != LG_DONE)) {
    const bool run = state != LG_DONE;
    // ---- one evaluation at the candidate theta: deviance, g, H, the smallest weight ----------------------------------------------------
    if (run) {
      for (int e = oG; e < oG + nq; ++e) LG(e) = 0.0;
      for (int e = oH; e < NS; ++e) LG(e) = 0.0;
      dev_e = 0.0;
      wmin = 1.0;
    }
    for (int64_t i = 0; i < n_ind; ++i) {
      if (!part[i]) continue;
      const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
      if (la < 0 || la >= A || lb < 0 || lb >= A) continue;
      if (!run) continue;
      const double* z = zy + i * K1;
      const bool same = la == lb;
      const int lo = la < lb ? la : lb, hi = la < lb ? lb : la;
      // the at most four columns besides Z that are not zero, in ascending column: h_lo, h_hi, d_lo, d_hi
      const int j1 = K + lo, j2 = K + hi, j3 = P + lo, j4 = P + hi;
      const double v1 = lo < Am1 ? (same ? 2.0 : 1.0) : 0.0;
      const double v2 = (!same && hi < Am1) ? 1.0 : 0.0;
      double v3 = 0.0, v4 = 0.0;
      if (!NULLFIT) {
        const int xa = as_code<KIND>(rows + (2 * i) * ld, c) == 1u, xb = as_code<KIND>(rows + (2 * i + 1) * ld, c) == 1u;
        const int dlo = same ? xa + xb : (la < lb ? xa : xb), dhi = same ? 0 : (la < lb ? xb : xa);
        v3 = ((keep >> lo) & 1u) ? (double)dlo : 0.0;
        v4 = ((keep >> hi) & 1u) ? (double)dhi : 0.0;
      }
      double eta = 0.0;
      for (int k = 0; k < K; ++k) eta += z[k] * LG(oTE + k);
      if (v1 != 0.0) eta += v1 * LG(oTE + j1);
      if (v2 != 0.0) eta += v2 * LG(oTE + j2);
      if (v3 != 0.0) eta += v3 * LG(oTE + j3);
      if (v4 != 0.0) eta += v4 * LG(oTE + j4);
      // e = exp(-|eta|): mu and 1 - mu without cancellation, w = e / (1 + e)^2, deviance term 2 (max(t, 0) + log1p(e)) with t = -eta for a
      // case and eta for a control
      const bool is_case = z[K] == 1.0;
      const double e = gnx_exp_sc(-fabs(eta));
      const double q = 1.0 / (1.0 + e), eq = e * q;
      const double r = is_case ? (eta >= 0.0 ? eq : q) : (eta >= 0.0 ? -q : -eq);   // y - mu
      const double w = eq * q;
      const double t = is_case ? -eta : eta;
      dev_e += 2.0 * ((t > 0.0 ? t : 0.0) + log1p(e));
      wmin = w < wmin ? w : wmin;
      for (int j = 0; j < K; ++j) {
        const double zj = z[j], wz = w * zj;
        LG(oG + j) += r * zj;
        const int base = oH + j * (j + 1) / 2;
        for (int k = 0; k <= j; ++k) LG(base + k) += wz * z[k];
      }
      const auto column = [&](int j, double v, int ja, double va, int jb, double vb, int jc, double vc) {
        const double wv = w * v;
        LG(oG + j) += r * v;
        const int base = oH + j * (j + 1) / 2;
        for (int k = 0; k < K; ++k) LG(base + k) += wv * z[k];
        if (va != 0.0) LG(base + ja) += wv * va;
        if (vb != 0.0) LG(base + jb) += wv * vb;
        if (vc != 0.0) LG(base + jc) += wv * vc;
        LG(base + j) += wv * v;
      };
      if (v1 != 0.0) column(j1, v1, 0, 0.0, 0, 0.0, 0, 0.0);
      if (v2 != 0.0) column(j2, v2, j1, v1, 0, 0.0, 0, 0.0);
      if (v3 != 0.0) column(j3, v3, j1, v1, j2, v2, 0, 0.0);
      if (v4 != 0.0) column(j4, v4, j1, v1, j2, v2, j3, v3);
    }
    // ---- the lane's next move --------------------------------------------------------------------------------------------------------------
    if (!run) {
      // (done: idles until the tile's last lane is)
    } else if (state == LG_INIT) {
      dev_cur = dev_e;
      state = LG_NEWTON;
    } else if (state == LG_LINE) {
      if (dev_e < dev_cur || halv == LG_MAX_HALVINGS) {
        for (int j = 0; j < nq; ++j) LG(oTH + j) = LG(oTE + j);
        dev_cur = dev_e;
        state = LG_NEWTON;
      } else {
        tstep *= 0.5;
        ++halv;
        for (int j = 0; j < nq; ++j) LG(oTE + j) = LG(oTH + j) + tstep * LG(oDL + j);
      }
    }
    const bool decide = run && (state == LG_NEWTON || state == LG_FINAL);   // (a rejected trial step stays in LG_LINE and is evaluated again)
    if (decide && state == LG_NEWTON && it == max_iter) {   // max_iter steps taken and the last one did not meet tol
      status = 3;
      state = LG_DONE;
    }
    if (decide && state != LG_DONE) {
      // H to unit diagonal (a dropped column: a unit row), then Cholesky in place, row by row
      bool notpd = false;
      for (int j = 0; j < nq; ++j) {
        const double d = LG(oH + j * (j + 1) / 2 + j);
        bool kept = j < K;
        if (j >= K && j < P) kept = (NULLFIT ? oi[2 + j - K] : wi[2 + j - K]) > 0;
        if (j >= P) kept = (keep >> (j - P)) & 1u;
        if (kept && !(d > 0.0)) notpd = true;
        LG(oS + j) = d > 0.0 ? sqrt(d) : 1.0;
      }
      for (int j = 0; j < nq; ++j) {
        const int rj = oH + j * (j + 1) / 2;
        const double sj = LG(oS + j);
        for (int k = 0; k <= j; ++k) {
          double sum = k < j ? LG(rj + k) / (sj * LG(oS + k)) : 1.0;
          const int rk = oH + k * (k + 1) / 2;
          for (int m = 0; m < k; ++m) sum -= LG(rj + m) * LG(rk + m);
          if (k < j) {
            LG(rj + k) = sum / LG(rk + k);
          } else {
            const bool okp = sum > LG_PIVOT_MIN && isfinite(sum);
            if (!okp) notpd = true;
            LG(rj + j) = sqrt(okp ? sum : 1.0);
          }
        }
      }
      if (notpd) {
        status = 1;
        state = LG_DONE;
      }
    }
    if (decide && state == LG_NEWTON) {
      // delta = H^-1 g through the factor of the scaled matrix; lambda^2 = g^T delta
      for (int j = 0; j < nq; ++j) {
        const int rj = oH + j * (j + 1) / 2;
        double sum = LG(oG + j) / LG(oS + j);
        for (int k = 0; k < j; ++k) sum -= LG(rj + k) * LG(oDL + k);
        LG(oDL + j) = sum / LG(rj + j);
      }
      for (int j = nq - 1; j >= 0; --j) {
        double sum = LG(oDL + j);
        for (int k = j + 1; k < nq; ++k) sum -= LG(oH + k * (k + 1) / 2 + j) * LG(oDL + k);
        LG(oDL + j) = sum / LG(oH + j * (j + 1) / 2 + j);
      }
      double lam = 0.0;
      for (int j = 0; j < nq; ++j) {
        const double dj = LG(oDL + j) / LG(oS + j);
        LG(oDL + j) = dj;
        lam += LG(oG + j) * dj;
      }
      ++it;
      tstep = 1.0;
      halv = 0;
      for (int j = 0; j < nq; ++j) LG(oTE + j) = LG(oTH + j) + LG(oDL + j);
      if (lam <= tol) {   // the full step, no deviance comparison; H once more at the returned theta
        for (int j = 0; j < nq; ++j) LG(oTH + j) = LG(oTE + j);
        state = LG_FINAL;
      } else {
        state = LG_LINE;
      }
    } else if (decide && state == LG_FINAL) {
      status = wmin < LG_W_MIN ? 3 : 0;
      if (status == 0) {
        if (NULLFIT) {
          for (int j = 0; j < P; ++j) of[j] = LG(oTH + j);
          of[P] = dev_e;
        } else {
          // se_j = sqrt((Hs^-1)_jj) / s_j; (Hs^-1)_jj = |L^-1 e_j|^2, the column solved forward into the step's slots
          for (int a = 0; a < A; ++a) {
            const int j = P + a;
            if (!((keep >> a) & 1u)) {
              of[a] = nan;
              of[A + a] = nan;
              continue;
            }
            double ss = 0.0;
            for (int k = j; k < nq; ++k) {
              const int rk = oH + k * (k + 1) / 2;
              double sum = k == j ? 1.0 : 0.0;
              for (int m = j; m < k; ++m) sum -= LG(rk + m) * LG(oDL + m);
              const double x = sum / LG(rk + k);
              LG(oDL + k) = x;
              ss += x * x;
            }
            of[a] = LG(oTH + j);
            of[A + a] = sqrt(ss) / LG(oS + j);
          }
          of[2 * A] = dev_e;
          if (oth)
            for (int j = 0; j < nq; ++j) oth[j] = LG(oTH + j);
        }
      }
      state = LG_DONE;
    }
  }
  if (active) {
    if (status != 0) {
      const int nf = NULLFIT ? L.WF : L.SF;
      for (int e = 0; e < nf; ++e) of[e] = nan;
      if (!NULLFIT && oth)
        for (int j = 0; j < nq; ++j) oth[j] = nan;
    }
    const int oi_it = NULLFIT ? A + 2 : 2 * A + 1;
    oi[oi_it] = it;
    oi[oi_it + 1] = status;
  }
#undef LG
#undef LGI
}

__global__ __launch_bounds__(LG_THREADS) void k_ancestry_assoc_logit_null(const int32_t* __restrict__ lab, int64_t ldl, int64_t n_ind, int A, int K,
                                                                          int64_t w0, const double* __restrict__ zy,
                                                                          const uint8_t* __restrict__ part, double tol, int max_iter,
                                                                          double* __restrict__ win_f, int32_t* __restrict__ win_i,
                                                                          unsigned long long* __restrict__ bad) {
  extern __shared__ double lg_lds[];   // [lg_slots(P)][1]
  const LgLayout L(A, K);
  lg_fit<GNX_ROWS_INT8, true>(lg_lds, 1, 0, threadIdx.x == 0, nullptr, 0, lab + w0 + blockIdx.x, ldl, n_ind, A, K, 0, zy, part, 1, tol, max_iter, nullptr,
                              nullptr, win_f + (int64_t)blockIdx.x * L.WF, win_i + (int64_t)blockIdx.x * L.WI, nullptr, bad);
}

template <int KIND>
__global__ __launch_bounds__(LG_THREADS) void k_ancestry_assoc_logit_snp(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lab,
                                                                         int64_t ldl, int64_t n_ind, int64_t C, int64_t M, int64_t W, int A, int K,
                                                                         int64_t c0, int64_t c1, int64_t w0, int64_t nw, int64_t tpw, int TC,
                                                                         const double* __restrict__ zy, const uint8_t* __restrict__ part, int min_ac,
                                                                         double tol, int max_iter, const double* __restrict__ win_f,
                                                                         const int32_t* __restrict__ win_i, double* __restrict__ snp_f,
                                                                         int32_t* __restrict__ snp_i, double* __restrict__ theta) {
  extern __shared__ double lg_lds[];   // [lg_slots(Q)][TC]
  const LgLayout L(A, K);
  // tiles are cut at window boundaries: block b serves tile b - wi tpw of window w0 + wi (the range's last window takes the rest)
  const int64_t b = blockIdx.x;
  const int64_t wi = b / tpw < nw - 1 ? b / tpw : nw - 1, w = w0 + wi;
  const int64_t cs = w * M + (b - wi * tpw) * TC, we = w == W - 1 ? C : (w + 1) * M;
  const int64_t c = cs + threadIdx.x;
  const bool active = (int)threadIdx.x < TC && c < we && c >= c0 && c < c1;
  const int64_t o = active ? c - c0 : 0;
  lg_fit<KIND, false>(lg_lds, TC, threadIdx.x < TC ? threadIdx.x : 0, active, rows, ld, lab + w, ldl, n_ind, A, K, c, zy, part, min_ac, tol, max_iter,
                      win_f + wi * L.WF, win_i + wi * L.WI, snp_f + o * L.SF, snp_i + o * L.SI, theta ? theta + o * L.Q : nullptr, nullptr);
}

int lg_tile_cols(int Q) {
  const size_t per = (size_t)lg_slots(Q) * 8;
  const size_t tc = LG_LDS_BYTES / per;
  return (int)(tc > (size_t)LG_THREADS ? LG_THREADS : tc);
}

// every refusal before the launch; GNX_OK or the code.  built: the rows are built by this call (the file path's form)
int logit_check(gnx_ctx* ctx, bool built, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N, int64_t C,
                int64_t M, int64_t W, int32_t A, const void* y, const void* Z, int32_t K, int32_t min_ac, int64_t c0, int64_t c1, double tol,
                int32_t max_iter, const void* snp_f64, const void* snp_i32, const void* win_f64, const void* win_i32) {
  const std::string w("ancestry_assoc_logit");
  const int rc = gnx_sum_geometry_check(ctx, "ancestry_assoc_logit", GNX_SUM_N_EVEN | GNX_SUM_OWN_NULLS, rows, row_kind, ld_rows, labels, ld_labels, N, C,
                                        M, W, A);
  if (rc != GNX_OK) return rc;
  if (K < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need K >= 1 covariates (the caller supplies the intercept column)");
  if (min_ac < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need min_ac >= 1");
  if (!(tol >= 0.0) || !std::isfinite(tol) || max_iter < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need a finite tol >= 0 and max_iter >= 1");
  if (c0 < 0 || c1 > C || c0 >= c1) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= c0 < c1 <= C");
  if ((!built && !rows) || !labels || !y || !Z || !snp_f64 || !snp_i32 || !win_f64 || !win_i32)
    return gnx_fail(ctx, GNX_EINVAL, w + ": a null pointer (only use, theta and n_bad may be NULL)");
  const int64_t Q = (int64_t)K + 2 * (int64_t)A - 1;
  if (K > GNX_ASSOC_MAX_K || Q > GNX_ASSOC_LOGIT_MAX_Q)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": K = " + std::to_string(K) + " covariates (at most " + std::to_string(GNX_ASSOC_MAX_K) + ") and Q = K + 2 A - 1 = " +
                                               std::to_string(Q) + " columns (at most " + std::to_string(GNX_ASSOC_LOGIT_MAX_Q) + ")");
  if (N > ((int64_t)1 << 28)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": N must not exceed 2^28 (the integer outputs are int32)");
  return GNX_OK;
}

const char* const LG_TAIL = "an individual with such a label takes no part at that window";

// prep, the verdict on y (GNX_EINVAL before any fit, nothing written), the null fits, the SNP fits, the verdict on the labels.
// Device pointers throughout; arguments checked by the caller.  Synchronises the stream twice.  *ran: the fits ran and the outputs are
// written (GNX_OK, or GNX_EINVAL for labels out of range).
int logit_run(gnx_ctx* ctx, const char* who, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N,
              int64_t C, int64_t M, int64_t W, int32_t A, const double* d_y, const double* d_Z, int32_t K, const uint8_t* d_use, int32_t min_ac,
              int64_t c0, int64_t c1, double tol, int32_t max_iter, double* d_snp_f64, int32_t* d_snp_i32, double* d_theta, double* d_win_f64,
              int32_t* d_win_i32, int64_t* n_bad, bool* ran) {
  hipStream_t s = ctx->stream;
  const LgLayout L(A, K);
  const int64_t n_ind = N / 2;
  *ran = false;
  struct {   // the workspace of one call: zy | part in ws_p64, the two counters (labels, phenotypes) in ws_misc
    double* zy;
    uint8_t* part;
    unsigned long long *d_bad, *d_bad_y;
  } wk;
  int rc;
  if ((rc = gnx_sum_zy_part(ctx, n_ind, K, &wk.zy, &wk.part)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 2, &wk.d_bad, s)) != GNX_OK) return rc;
  wk.d_bad_y = wk.d_bad + 1;
  if (n_bad) *n_bad = 0;
  unsigned long long h_bad[2] = {0, 0};
  if (n_ind > 0) {
    hipLaunchKernelGGL(k_ancestry_assoc_logit_prep, dim3((unsigned)((n_ind + 255) / 256)), dim3(256), 0, s, d_y, d_Z, d_use, n_ind, (int)K, wk.zy, wk.part,
                       wk.d_bad_y);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(h_bad, wk.d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_bad[1]) {
      if (n_bad) *n_bad = (int64_t)h_bad[1];
      return gnx_fail(ctx, GNX_EINVAL, std::string(who) + ": " + std::to_string(h_bad[1]) +
                                           " individuals with use != 0 have a phenotype that is neither 0 nor 1 (a case / control trait is coded 0 / 1)");
    }
  }
  const int64_t w0 = as_win(c0, M, W), w1 = as_win(c1 - 1, M, W), nw = w1 - w0 + 1;
  const size_t lds0 = (size_t)lg_slots(L.P) * 8;
  hipLaunchKernelGGL(k_ancestry_assoc_logit_null, dim3((unsigned)nw), dim3(LG_THREADS), lds0, s, d_labels, ld_labels, n_ind, (int)A, (int)K, w0, wk.zy,
                     wk.part, tol, (int)max_iter, d_win_f64, d_win_i32, wk.d_bad);
  HIPCHK(ctx, hipGetLastError());
  const int tc = lg_tile_cols(L.Q);
  const size_t lds = (size_t)tc * lg_slots(L.Q) * 8;
  const int64_t tpw = (M + tc - 1) / tc;
  const int64_t last_w = (w1 == W - 1 ? C : (w1 + 1) * M) - w1 * M;
  const int64_t nblocks = (nw - 1) * tpw + (last_w + tc - 1) / tc;
  if (nblocks > 0x7fffffff) return gnx_fail(ctx, GNX_EUNSUPPORTED, std::string(who) + ": too many tiles for one launch; call with a shorter [c0, c1)");
  const uint8_t* rows = (const uint8_t*)d_rows;
  if (row_kind == GNX_ROWS_PACKED2) {
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ancestry_assoc_logit_snp<GNX_ROWS_PACKED2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)LG_LDS_BYTES));
    hipLaunchKernelGGL(k_ancestry_assoc_logit_snp<GNX_ROWS_PACKED2>, dim3((unsigned)nblocks), dim3(LG_THREADS), lds, s, rows, ld_rows, d_labels, ld_labels,
                       n_ind, C, M, W, (int)A, (int)K, c0, c1, w0, nw, tpw, tc, wk.zy, wk.part, (int)min_ac, tol, (int)max_iter, d_win_f64, d_win_i32,
                       d_snp_f64, d_snp_i32, d_theta);
  } else {
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ancestry_assoc_logit_snp<GNX_ROWS_INT8>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)LG_LDS_BYTES));
    hipLaunchKernelGGL(k_ancestry_assoc_logit_snp<GNX_ROWS_INT8>, dim3((unsigned)nblocks), dim3(LG_THREADS), lds, s, rows, ld_rows, d_labels, ld_labels, n_ind,
                       C, M, W, (int)A, (int)K, c0, c1, w0, nw, tpw, tc, wk.zy, wk.part, (int)min_ac, tol, (int)max_iter, d_win_f64, d_win_i32, d_snp_f64,
                       d_snp_i32, d_theta);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(h_bad, wk.d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *ran = true;
  return gnx_sum_label_verdict(ctx, who, h_bad[0], A, LG_TAIL, n_bad);
}

// host outputs of one call, staged in ws_b64 / ws_b32
struct LgOut {
  size_t sf, si, st, wf, wi;
  double *d_sf, *d_th, *d_wf;
  int32_t *d_si, *d_wi;
};

int logit_out(gnx_ctx* ctx, int32_t A, int32_t K, int64_t nc, int64_t nw, bool want_theta, LgOut* o) {
  const LgLayout L(A, K);
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  o->sf = (size_t)nc * L.SF * 8;
  o->si = (size_t)nc * L.SI * 4;
  o->st = want_theta ? (size_t)nc * L.Q * 8 : 0;
  o->wf = (size_t)nw * L.WF * 8;
  o->wi = (size_t)nw * L.WI * 4;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b64, up(o->sf) + up(o->st) + o->wf + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b32, up(o->si) + o->wi + 64)) != GNX_OK) return rc;
  char* b64 = (char*)ctx->ws_b64.p;
  o->d_sf = (double*)b64;
  o->d_th = want_theta ? (double*)(b64 + up(o->sf)) : nullptr;
  o->d_wf = (double*)(b64 + up(o->sf) + up(o->st));
  o->d_si = (int32_t*)ctx->ws_b32.p;
  o->d_wi = (int32_t*)((char*)ctx->ws_b32.p + up(o->si));
  return GNX_OK;
}

int logit_copy_out(gnx_ctx* ctx, const LgOut& o, double* snp_f64, int32_t* snp_i32, double* theta, double* win_f64, int32_t* win_i32) {
  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(snp_f64, o.d_sf, o.sf, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(snp_i32, o.d_si, o.si, hipMemcpyDeviceToHost, s));
  if (theta) HIPCHK(ctx, hipMemcpyAsync(theta, o.d_th, o.st, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_f64, o.d_wf, o.wf, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_i32, o.d_wi, o.wi, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_ancestry_assoc_logit_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                            int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_y, const double* d_Z, int32_t K,
                                            const uint8_t* d_use, int32_t min_ac, int64_t c0, int64_t c1, double tol, int32_t max_iter,
                                            double* d_snp_f64, int32_t* d_snp_i32, double* d_theta, double* d_win_f64, int32_t* d_win_i32,
                                            int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = logit_check(ctx, false, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_y, d_Z, K, min_ac, c0, c1, tol, max_iter, d_snp_f64,
                       d_snp_i32, d_win_f64, d_win_i32);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  bool ran;
  return logit_run(ctx, "ancestry_assoc_logit", d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_y, d_Z, K, d_use, min_ac, c0, c1, tol,
                   max_iter, d_snp_f64, d_snp_i32, d_theta, d_win_f64, d_win_i32, n_bad, &ran);
}


namespace {
// the tail the two host forms share: the fits over DEVICE rows and labels with the staged phenotypes, then the outputs -> the host.
// GNX_EINVAL for labels out of range (the fits ran): the results stand and are handed over; any other failure leaves the outputs alone.
int logit_host_run(gnx_ctx* ctx, const char* who, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N,
                   int64_t C, int64_t M, int64_t W, int32_t A, const gnx_sum_pheno& ph, int32_t K, int32_t min_ac, int64_t c0, int64_t c1, double tol,
                   int32_t max_iter, const LgOut& o, double* snp_f64, int32_t* snp_i32, double* theta, double* win_f64, int32_t* win_i32,
                   int64_t* n_bad) {
  int64_t nbad = 0;
  bool ran;
  const int rc = logit_run(ctx, who, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, ph.d_y, ph.d_Z, K, ph.d_use, min_ac, c0, c1, tol,
                           max_iter, o.d_sf, o.d_si, o.d_th, o.d_wf, o.d_wi, &nbad, &ran);
  if (n_bad) *n_bad = nbad;
  if (!ran) return rc;
  const std::string msg = ctx->err;
  const int rc2 = logit_copy_out(ctx, o, snp_f64, snp_i32, theta, win_f64, win_i32);
  if (rc2 != GNX_OK) return rc2;
  ctx->err = msg;
  return rc;
}
}  // namespace

extern "C" int gnx_ancestry_assoc_logit(gnx_ctx* ctx, const int8_t* X, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t C,
                                        int64_t M, int64_t W, int32_t A, const double* y, const double* Z, int32_t K, const uint8_t* use,
                                        int32_t min_ac, int64_t c0, int64_t c1, double tol, int32_t max_iter, double* snp_f64, int32_t* snp_i32,
                                        double* theta, double* win_f64, int32_t* win_i32, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = logit_check(ctx, false, X, GNX_ROWS_INT8, ld_rows, labels, ld_labels, N, C, M, W, A, y, Z, K, min_ac, c0, c1, tol, max_iter, snp_f64, snp_i32,
                       win_f64, win_i32);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  // inputs: rows -> ws_xu, labels -> ws_lab, y | Z | use -> ws_scale; outputs: float64 in ws_b64, int32 in ws_b32
  gnx_sum_pheno ph;
  LgOut o;
  if ((rc = gnx_sum_stage_rows_labels(ctx, X, GNX_ROWS_INT8, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_stage_pheno(ctx, y, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  if ((rc = logit_out(ctx, A, K, c1 - c0, as_win(c1 - 1, M, W) - as_win(c0, M, W) + 1, theta != nullptr, &o)) != GNX_OK) return rc;
  return logit_host_run(ctx, "ancestry_assoc_logit", ctx->ws_xu.p, GNX_ROWS_INT8, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, ph, K,
                        min_ac, c0, c1, tol, max_iter, o, snp_f64, snp_i32, theta, win_f64, win_i32, n_bad);
}

// The file path's form.  A Newton step needs every individual, so the packed rows of ALL individuals are built in HBM first
// (N rows of gnx_sum_gt2's pitch, batch by batch with gnx_infer_gt2's staging: GNX_HOST_BATCH only governs how they are built), then the
// fits run once over them: the results are gnx_ancestry_assoc_logit's of the vcf_to_npy matrix bit for bit.
extern "C" int gnx_ancestry_assoc_logit_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src,
                                            const int32_t* labels, const double* y, const double* Z, int32_t K, const uint8_t* use, int32_t min_ac,
                                            int64_t c0, int64_t c1, double tol, int32_t max_iter, double* snp_f64, int32_t* snp_i32, double* theta,
                                            double* win_f64, int32_t* win_i32, int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  int rc = gnx_sum_gt2_args(ctx, "ancestry_assoc_logit_gt2", G, V, ldg, N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = logit_check(ctx, true, nullptr, GNX_ROWS_PACKED2, (C + 3) / 4, labels, W, N, C, M, W, A, y, Z, K, min_ac, c0, c1, tol, max_iter, snp_f64,
                        snp_i32, win_f64, win_i32)) != GNX_OK)
    return rc;
  if ((rc = gnx_sum_check_src(ctx, "ancestry_assoc_logit_gt2", src, C, V)) != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  gnx_sum_gt2 st;
  gnx_sum_pheno ph;
  LgOut o;
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, false, &st, s)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_xu, (size_t)N * st.ldp + 256)) != GNX_OK) return rc;
  if ((rc = gnx_sum_stage_pheno(ctx, y, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  if ((rc = logit_out(ctx, A, K, c1 - c0, as_win(c1 - 1, M, W) - as_win(c0, M, W) + 1, theta != nullptr, &o)) != GNX_OK) return rc;
  HIPCHK(ctx, gnx_sum_gt2_all_rows(st, N, C, ctx->ws_xu.p, s));
  return logit_host_run(ctx, "ancestry_assoc_logit_gt2", ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab, W, N, C, M, W, A, ph, K, min_ac, c0, c1, tol,
                        max_iter, o, snp_f64, snp_i32, theta, win_f64, win_i32, n_bad);
}
