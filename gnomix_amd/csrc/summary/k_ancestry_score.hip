// summary/k_ancestry_score.hip — ancestry-partitioned polygenic scores ("partial PRS") in one fused pass over X and the labels: for
// individual i (haplotype rows 2 i, 2 i + 1), ancestry a and score s, the sum of weights[c, a, s] over the scored SNPs c and the
// individual's haplotypes h with labels[h, win(c)] == a and X[h, c] == effect[c].  The per-ancestry dosage matrices of
// k_allele_counts.hip are never materialised.
//
// Inputs as gnx_ancestry_allele_counts takes them (rows int8 or 2-bit, labels (N, W) int32, win(c) = min(c / M, W - 1)), plus
// weights (C, A, S) float64 and effect (C,) uint8: 1 = the effect allele is ALT, 0 = REF, 255 = the SNP is not scored.
//
// SUMMATION ORDER (float64; the integers are exact).  Two levels, a function of (C, M, W) alone:
//   1. per haplotype h and window k whose label a = labels[h, k] lies in [0, A): a partial p[h, k, s] starts at +0.0 and adds
//      weights[c, a, s] for the SNPs c of window k in ASCENDING c with effect[c] != 255 and X[h, c] == effect[c];
//   2. per (i, a, s): score starts at +0.0 and adds, in ASCENDING k, first p[2 i, k, s] if labels[2 i, k] == a, then p[2 i + 1, k, s] if
//      labels[2 i + 1, k] == a.
// One rounding per add, no fused multiply-add (there is no multiply), terms that do not apply are skipped.  A partial that met no
// SNP is +0.0 and is added all the same: x + (+0.0) == x bit for bit for every x a sum can hold here, since a sum that starts at +0.0
// never becomes -0.0 under round-to-nearest.  The order does not depend on N, the grid, the tiles below, the row form, the passes over
// row ranges, the file path's batches or the debug arguments.
//
// k_ancestry_score_check: effect bytes outside {0, 1, 255} and non-finite weights at scored SNPs, counted before anything is written.
// k_ancestry_score_partial<KIND, SB>: level 1.  A workgroup is 256 threads = a tile of SC_ROWS = 256 haplotypes (lane = haplotype) x a
//   range of windows; it walks the columns of its windows in chunks of COLS = 16 GROUPS columns that start at multiples of COLS (256
//   columns of int8 rows, 512 of packed rows: 128 packed bytes or 256 int8 bytes of every row per chunk).  The chunk is staged in LDS
//   coalesced, as ONE dword of 16 2-bit fields per (row, 16 columns) whatever the row form (as_fields16: a 16-byte load of an int8 row,
//   a 4-byte load of a packed row; X is read from HBM once, never byte by byte on aligned rows), rows GROUPS + 1 dwords apart (an odd
//   stride: the lanes' reads of their own rows are conflict-free).  The chunk's effect bytes become two masks per 16 columns (scored,
//   effect allele) in LDS.  The weights of the chunk are staged in sub-chunks of WC columns (the largest power of two with
//   WC A SB 8 <= 32 KiB), [column][ancestry][SB] float64 with the S scores padded to SB in {1, 2, 4, 8, 16} by zeros, so the lane's SB
//   accumulators are registers with compile-time indices.  A lane tests 16 columns with a few bit operations (match = scored & ~missing
//   & ~(alt ^ effect)), counts with popcounts and adds the matching columns' weights of ITS ancestry in ascending column.  Where a window
//   ends the lane stores its partial, three counts and its label as a byte (0xff outside [0, A)) to the workspace, [window][..][row]
//   (adjacent lanes, adjacent addresses), and goes on with the next window's label.  Labels are only compared, never used as an index
//   before the range test.  LDS: <= 32 KiB weights + <= 33 KiB tile: two workgroups per CU.
// k_ancestry_score_reduce: level 2.  One thread per (individual, ancestry, score) walks the windows in ascending k over the workspace
//   (coalesced: adjacent threads = adjacent individuals) and owns its output: plain stores, nothing to zero.  The thread of score 0
//   also sums the three counts.
// Rows go in passes of at most SC_WS_BYTES of partials (a multiple of SC_ROWS rows each); the order is per individual, so passes
// change nothing.  No per-thread array is indexed at run time; no scratch.
#include "gnx_summary_host.h"

namespace {

constexpr int SC_ROWS = 256;                       // haplotypes per workgroup = threads
constexpr int SC_RED_THREADS = 64;
constexpr size_t SC_W_BYTES = 32 * 1024;           // staged weights of one sub-chunk
constexpr size_t SC_WS_BYTES = (size_t)256 << 20;  // partials of one pass over rows
constexpr int SC_MAX_A = GNX_ALLELE_MAX_A;
constexpr int SC_MAX_S = GNX_SCORE_MAX_S;
constexpr uint32_t SC_EVEN = 0x55555555u;

template <int KIND>
struct ScTile {
  static constexpr int GROUPS = KIND == GNX_ROWS_PACKED2 ? 32 : 16;  // groups of 16 columns per chunk
  static constexpr int COLS = GROUPS * 16;
  static constexpr int LD = GROUPS + 1;                              // dwords between two rows of the staged tile
};

__global__ __launch_bounds__(256) void k_ancestry_score_check(const double* __restrict__ weights, const uint8_t* __restrict__ effect, int64_t C,
                                                              int64_t AS, unsigned long long* __restrict__ bad) {
  unsigned int bad_e = 0, bad_w = 0;
  const int64_t total = C * AS;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / AS;
    const uint8_t f = effect[c];
    if (f != 255 && !isfinite(weights[e])) ++bad_w;
    if (e == c * AS && f > 1 && f != 255) ++bad_e;
  }
  if (bad_e) atomicAdd(bad + 1, (unsigned long long)bad_e);
  if (bad_w) atomicAdd(bad + 2, (unsigned long long)bad_w);
}

// rows, lab: of the pass's first row; n rows in the pass.  Workspace of the pass: part [W][S][n] float64, cnt [W][3][n] int32 (effect,
// scored, missing), lab8 [W][n] bytes.
template <int KIND, int SB>
__global__ __launch_bounds__(SC_ROWS) void k_ancestry_score_partial(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lab,
                                                                    int64_t ldl, int64_t n, int64_t C, int64_t M, int64_t W, int A, int S,
                                                                    const double* __restrict__ weights, const uint8_t* __restrict__ effect,
                                                                    int64_t n_rtiles, int64_t wpb, int WC, int aligned,
                                                                    double* __restrict__ part, int32_t* __restrict__ cnt,
                                                                    uint8_t* __restrict__ lab8, unsigned long long* __restrict__ bad) {
  using T = ScTile<KIND>;
  extern __shared__ double sc_lds[];     // weights [WC][A][SB] float64; the tile [SC_ROWS][LD] dwords; the masks [2][GROUPS] dwords
  double* wl = sc_lds;
  uint32_t* xt = reinterpret_cast<uint32_t*>(sc_lds + (size_t)WC * A * SB);
  uint32_t* msc = xt + SC_ROWS * T::LD;
  uint32_t* mef = msc + T::GROUPS;
  const int tid = threadIdx.x;
  const int64_t rt = blockIdx.x % n_rtiles, wr = blockIdx.x / n_rtiles;
  const int64_t h0 = rt * SC_ROWS, hl = h0 + tid;        // this lane's row within the pass
  const bool live = hl < n;
  const int64_t k0 = wr * wpb, k1 = (k0 + wpb < W) ? k0 + wpb : W;          // the windows [k0, k1), k1 > k0 by the grid
  const int64_t cbeg = k0 * M, cend = (k1 == W) ? C : k1 * M;               // their columns
  const int ASB = A * SB;
  int64_t k = k0, wend = (k == W - 1) ? C : (k + 1) * M;
  int a = -1;
  if (live) {
    const int32_t v = lab[hl * ldl + k];
    a = (v >= 0 && v < A) ? v : -1;
  }
  double acc[SB];
#pragma unroll
  for (int s = 0; s < SB; ++s) acc[s] = 0.0;
  int ne = 0, ns = 0, nm = 0;
  unsigned int my_bad = 0;

  for (int64_t t0 = cbeg / T::COLS * T::COLS; t0 < cend; t0 += T::COLS) {
    __syncthreads();                     // the chunk before is read
    for (int e = tid; e < SC_ROWS * T::GROUPS; e += SC_ROWS) {
      const int r = e / T::GROUPS, g = e - r * T::GROUPS;
      const int64_t c0 = t0 + 16 * g;
      uint32_t f = 0;
      if (h0 + r < n && c0 < C) f = as_fields16<KIND>(rows + (h0 + r) * ld, c0, C, aligned);
      xt[r * T::LD + g] = f;
    }
    if (tid < T::GROUPS) {               // the effect bytes of 16 columns -> two masks at the even bits (columns >= C are not scored)
      uint32_t sb = 0, eb = 0;
      const int64_t c0 = t0 + 16 * tid;
      for (int j = 0; j < 16 && c0 + j < C; ++j) {
        const uint32_t f = effect[c0 + j];
        if (f != 255u) sb |= 1u << (2 * j);
        if (f == 1u) eb |= 1u << (2 * j);
      }
      msc[tid] = sb;
      mef[tid] = eb;
    }
    const int64_t t1 = (t0 + T::COLS < cend) ? t0 + T::COLS : cend;
    for (int64_t u0 = t0; u0 < t1; u0 += WC) {
      if (u0 + WC <= cbeg) continue;     // (uniform) a sub-chunk before the range's first column
      __syncthreads();                   // the tile is staged; the weights before are read
      {
        const int64_t ncol = (C - u0 < WC) ? C - u0 : WC;
        const int nel = (int)ncol * ASB;
        if (SB == S) {                   // no padding: one contiguous copy
          const double* src = weights + u0 * ASB;
          for (int e = tid; e < nel; e += SC_ROWS) wl[e] = src[e];
        } else {
          for (int e = tid; e < nel; e += SC_ROWS) {
            const int q = e / SB, s = e - q * SB;   // q = column * A + ancestry
            wl[e] = s < S ? weights[(u0 * A + q) * S + s] : 0.0;
          }
        }
      }
      __syncthreads();
      int64_t c = u0 > cbeg ? u0 : cbeg;
      const int64_t ue = (u0 + WC < t1) ? u0 + WC : t1;
      while (c < ue) {
        const int64_t se = ue < wend ? ue : wend;   // the columns [c, se) lie in window k
        if (a >= 0) {
          for (int64_t g0 = c & ~(int64_t)15; g0 < se; g0 += 16) {
            const int gi = (int)((g0 - t0) >> 4);
            const uint32_t f = xt[tid * T::LD + gi];
            const int lo = (int)(c > g0 ? c - g0 : 0), hi = (int)(se - g0 < 16 ? se - g0 : 16);
            const uint32_t sc = msc[gi] & as_range16(lo, hi);
            const uint32_t miss = (f >> 1) & SC_EVEN, alt = f & SC_EVEN & ~miss;
            const uint32_t mt = sc & ~miss & ~(alt ^ mef[gi]);
            nm += __popc(sc & miss);
            ns += __popc(sc & ~miss);
            ne += __popc(mt);
            if (mt) {
              const int off = ((int)(g0 - u0) * A + a) * SB;     // (negative where g0 < u0: only the columns >= c >= u0 are read)
#pragma unroll
              for (int j = 0; j < 16; ++j) {
                if ((mt >> (2 * j)) & 1u) {
                  const double* w = wl + (off + j * ASB);
#pragma unroll
                  for (int s = 0; s < SB; ++s) acc[s] += w[s];
                }
              }
            }
          }
        }
        c = se;
        if (c == wend && c < cend) {     // (uniform) the window ends inside the range: store it and go on with the next
          if (live) {
            const int64_t o = k * n + hl;
            lab8[o] = a >= 0 ? (uint8_t)a : (uint8_t)0xff;
            cnt[(k * 3 + 0) * n + hl] = ne;
            cnt[(k * 3 + 1) * n + hl] = ns;
            cnt[(k * 3 + 2) * n + hl] = nm;
#pragma unroll
            for (int s = 0; s < SB; ++s)
              if (s < S) part[(k * S + s) * n + hl] = acc[s];
            if (a < 0) ++my_bad;
          }
          ++k;
          wend = (k == W - 1) ? C : wend + M;
          a = -1;
          if (live) {
            const int32_t v = lab[hl * ldl + k];
            a = (v >= 0 && v < A) ? v : -1;
          }
#pragma unroll
          for (int s = 0; s < SB; ++s) acc[s] = 0.0;
          ne = ns = nm = 0;
        }
      }
    }
  }
  if (live) {                            // the range's last window
    const int64_t o = k * n + hl;
    lab8[o] = a >= 0 ? (uint8_t)a : (uint8_t)0xff;
    cnt[(k * 3 + 0) * n + hl] = ne;
    cnt[(k * 3 + 1) * n + hl] = ns;
    cnt[(k * 3 + 2) * n + hl] = nm;
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s < S) part[(k * S + s) * n + hl] = acc[s];
    if (a < 0) ++my_bad;
  }
  if (my_bad) atomicAdd(bad, (unsigned long long)my_bad);
}

// outputs: of the pass's first individual; any may be NULL
__global__ __launch_bounds__(SC_RED_THREADS) void k_ancestry_score_reduce(const double* __restrict__ part, const int32_t* __restrict__ cnt,
                                                                          const uint8_t* __restrict__ lab8, int64_t n, int64_t W, int A, int S,
                                                                          int64_t n_itiles, double* __restrict__ score,
                                                                          int32_t* __restrict__ n_effect, int32_t* __restrict__ n_scored,
                                                                          int32_t* __restrict__ n_miss) {
  const int64_t i = (blockIdx.x % n_itiles) * SC_RED_THREADS + threadIdx.x;
  const int q = (int)(blockIdx.x / n_itiles), a = q / S, s = q - a * S;
  if (2 * i >= n) return;
  const bool ints = s == 0 && (n_effect || n_scored || n_miss);
  double acc = 0.0;
  int ne = 0, ns = 0, nm = 0;
  for (int64_t k = 0; k < W; ++k) {
    const int64_t o = k * n + 2 * i;
    const int la = lab8[o], lb = lab8[o + 1];
    if (la == a) {
      if (score) acc += part[(k * S + s) * n + 2 * i];
      if (ints) {
        ne += cnt[(k * 3 + 0) * n + 2 * i];
        ns += cnt[(k * 3 + 1) * n + 2 * i];
        nm += cnt[(k * 3 + 2) * n + 2 * i];
      }
    }
    if (lb == a) {
      if (score) acc += part[(k * S + s) * n + 2 * i + 1];
      if (ints) {
        ne += cnt[(k * 3 + 0) * n + 2 * i + 1];
        ns += cnt[(k * 3 + 1) * n + 2 * i + 1];
        nm += cnt[(k * 3 + 2) * n + 2 * i + 1];
      }
    }
  }
  if (score) score[(i * A + a) * S + s] = acc;
  if (ints) {
    if (n_effect) n_effect[i * A + a] = ne;
    if (n_scored) n_scored[i * A + a] = ns;
    if (n_miss) n_miss[i * A + a] = nm;
  }
}

int sc_pad(int S) { return S <= 1 ? 1 : S <= 2 ? 2 : S <= 4 ? 4 : S <= 8 ? 8 : 16; }

// columns of a weight sub-chunk: the largest power of two <= the chunk with WC A SB 8 <= SC_W_BYTES (>= 8 at A = 32, SB = 16)
int sc_wcols(int cols, int A, int SB) {
  int wc = cols;
  while (wc > 1 && (size_t)wc * A * SB * 8 > SC_W_BYTES) wc >>= 1;
  return wc;
}

const char* const SC_TAIL = "such a haplotype counts for no ancestry at that window";

// every refusal that needs no device memory; GNX_OK or the code.  built: the rows are built by this call (the file path's form)
int score_check(gnx_ctx* ctx, const char* who, bool built, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels,
                int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const void* weights, int32_t S, const void* effect, int64_t dbg_wpb,
                int64_t dbg_rpp) {
  const std::string w(who);
  const int rc = gnx_sum_geometry_check(ctx, who, GNX_SUM_N_EVEN | (built ? GNX_SUM_ROWS_BUILT : 0u), rows, row_kind, ld_rows, labels, ld_labels, N, C, M,
                                        W, A);
  if (rc != GNX_OK) return rc;
  if (S < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need S >= 1 scores");
  if (!weights || !effect) return gnx_fail(ctx, GNX_EINVAL, w + ": no weights or no effect alleles");
  if (N >= ((int64_t)1 << 31)) return gnx_fail(ctx, GNX_EINVAL, w + ": N must be below 2^31");
  if (dbg_wpb < 0 || dbg_rpp < 0) return gnx_fail(ctx, GNX_EINVAL, w + ": the debug arguments must be >= 0 (0 = the built-in choice)");
  if (A > SC_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, at most " + std::to_string(SC_MAX_A));
  if (S > SC_MAX_S) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": S = " + std::to_string(S) + " scores per call, at most " + std::to_string(SC_MAX_S));
  if (C >= ((int64_t)1 << 30)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": C must be below 2^30 (the counts are int32)");
  return GNX_OK;
}

// the checking pass over DEVICE weights and effect: GNX_EINVAL names the count.  d_bad: three zeroed slots (labels, effect bytes, weights).
// Synchronises.
int score_verify(gnx_ctx* ctx, const char* who, const double* d_weights, const uint8_t* d_effect, int64_t C, int32_t A, int32_t S,
                 unsigned long long* d_bad, hipStream_t s) {
  const int64_t AS = (int64_t)A * S, total = C * AS;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL(k_ancestry_score_check, dim3(grid), dim3(256), 0, s, d_weights, d_effect, C, AS, d_bad);
  HIPCHK(ctx, hipGetLastError());
  unsigned long long h[3] = {0, 0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h, d_bad, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (h[1]) return gnx_fail(ctx, GNX_EINVAL, std::string(who) + ": " + std::to_string(h[1]) + " effect bytes are none of 0 (REF), 1 (ALT), 255 (not scored)");
  if (h[2]) return gnx_fail(ctx, GNX_EINVAL, std::string(who) + ": " + std::to_string(h[2]) + " weights at scored SNPs are not finite");
  return GNX_OK;
}

template <int KIND, int SB>
hipError_t score_launch_partial(const uint8_t* rows, int64_t ld, const int32_t* lab, int64_t ldl, int64_t n, int64_t C, int64_t M, int64_t W, int A,
                                int S, const double* w, const uint8_t* eff, int64_t n_rtiles, int64_t wpb, int aligned, double* part, int32_t* cnt,
                                uint8_t* lab8, unsigned long long* bad, hipStream_t s) {
  using T = ScTile<KIND>;
  const int WC = sc_wcols(T::COLS, A, SB);
  const size_t lds = (size_t)WC * A * SB * 8 + ((size_t)SC_ROWS * T::LD + 2 * T::GROUPS) * 4;
  const int64_t n_wr = (W + wpb - 1) / wpb;
  if (n_wr > (((int64_t)1 << 31) - 1) / n_rtiles) return hipErrorInvalidConfiguration;
  GNX_LDS_OPTIN(lds, k_ancestry_score_partial<KIND, SB>);
  hipLaunchKernelGGL((k_ancestry_score_partial<KIND, SB>), dim3((unsigned)(n_rtiles * n_wr)), dim3(SC_ROWS), lds, s, rows, ld, lab, ldl, n, C, M, W, A,
                     S, w, eff, n_rtiles, wpb, WC, aligned, part, cnt, lab8, bad);
  return hipGetLastError();
}

template <int KIND>
hipError_t score_launch_kind(int SB, const uint8_t* rows, int64_t ld, const int32_t* lab, int64_t ldl, int64_t n, int64_t C, int64_t M, int64_t W,
                             int A, int S, const double* w, const uint8_t* eff, int64_t n_rtiles, int64_t wpb, int aligned, double* part,
                             int32_t* cnt, uint8_t* lab8, unsigned long long* bad, hipStream_t s) {
  switch (SB) {
    case 1: return score_launch_partial<KIND, 1>(rows, ld, lab, ldl, n, C, M, W, A, S, w, eff, n_rtiles, wpb, aligned, part, cnt, lab8, bad, s);
    case 2: return score_launch_partial<KIND, 2>(rows, ld, lab, ldl, n, C, M, W, A, S, w, eff, n_rtiles, wpb, aligned, part, cnt, lab8, bad, s);
    case 4: return score_launch_partial<KIND, 4>(rows, ld, lab, ldl, n, C, M, W, A, S, w, eff, n_rtiles, wpb, aligned, part, cnt, lab8, bad, s);
    case 8: return score_launch_partial<KIND, 8>(rows, ld, lab, ldl, n, C, M, W, A, S, w, eff, n_rtiles, wpb, aligned, part, cnt, lab8, bad, s);
    default: return score_launch_partial<KIND, 16>(rows, ld, lab, ldl, n, C, M, W, A, S, w, eff, n_rtiles, wpb, aligned, part, cnt, lab8, bad, s);
  }
}

// bytes of one row's share of a pass's workspace: partials, counts, the label byte
size_t sc_row_bytes(int64_t W, int S) { return (size_t)W * ((size_t)S * 8 + 3 * 4 + 1); }

// rows of one pass: a multiple of SC_ROWS whose partials stay within SC_WS_BYTES (at least SC_ROWS)
int64_t sc_rows_per_pass(int64_t N, int64_t W, int S, int64_t dbg_rpp) {
  int64_t rp = dbg_rpp > 0 ? dbg_rpp : (int64_t)(SC_WS_BYTES / sc_row_bytes(W, S));
  rp = std::max<int64_t>(SC_ROWS, rp / SC_ROWS * SC_ROWS);
  return std::min(rp, (N + SC_ROWS - 1) / SC_ROWS * SC_ROWS);
}

int score_reserve(gnx_ctx* ctx, int64_t rp, int64_t W, int S) {
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_p64, (size_t)rp * W * S * 8 + 256)) != GNX_OK) return rc;
  return gnx_ws_reserve(ctx, ctx->ws_p32, (size_t)rp * W * 13 + 512);
}

// both levels over N > 0 rows (rows, labels and outputs of THOSE rows' individuals), pass by pass; adds the labels out of range to
// d_bad[0].  Arguments checked and the workspaces reserved (score_reserve with the same rp) by the caller.
hipError_t score_launch(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N,
                        int64_t C, int64_t M, int64_t W, int32_t A, const double* d_w, int32_t S, const uint8_t* d_eff, double* d_score,
                        int32_t* d_ne, int32_t* d_ns, int32_t* d_nm, int64_t dbg_wpb, int64_t rp, unsigned long long* d_bad, hipStream_t s) {
  const int SB = sc_pad(S);
  const int aligned = gnx_sum_rows_aligned(d_rows, row_kind, ld_rows);
  double* part = (double*)ctx->ws_p64.p;
  int32_t* cnt = (int32_t*)ctx->ws_p32.p;
  for (int64_t r0 = 0; r0 < N; r0 += rp) {
    const int64_t n = std::min(rp, N - r0);      // even: rp is a multiple of SC_ROWS and N is even
    uint8_t* lab8 = (uint8_t*)ctx->ws_p32.p + (((size_t)n * W * 12 + 255) & ~(size_t)255);
    const int64_t n_rtiles = (n + SC_ROWS - 1) / SC_ROWS;
    int64_t wpb = dbg_wpb;
    if (wpb <= 0) {                              // about eight workgroups per CU
      const int64_t ranges = std::max<int64_t>(1, ((int64_t)ctx->n_cu * 8 + n_rtiles - 1) / n_rtiles);
      wpb = std::max<int64_t>(1, (W + ranges - 1) / ranges);
    }
    wpb = std::min(wpb, W);
    const uint8_t* rows = (const uint8_t*)d_rows + r0 * ld_rows;
    const int32_t* lab = d_labels + r0 * ld_labels;
    if (row_kind == GNX_ROWS_PACKED2)
      GNX_HIPRET((score_launch_kind<GNX_ROWS_PACKED2>(SB, rows, ld_rows, lab, ld_labels, n, C, M, W, A, S, d_w, d_eff, n_rtiles, wpb, aligned, part, cnt,
                                                      lab8, d_bad, s)));
    else
      GNX_HIPRET((score_launch_kind<GNX_ROWS_INT8>(SB, rows, ld_rows, lab, ld_labels, n, C, M, W, A, S, d_w, d_eff, n_rtiles, wpb, aligned, part, cnt,
                                                   lab8, d_bad, s)));
    const int64_t i0 = r0 / 2, n_itiles = (n / 2 + SC_RED_THREADS - 1) / SC_RED_THREADS;
    if (n_itiles > (((int64_t)1 << 31) - 1) / ((int64_t)A * S)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_ancestry_score_reduce, dim3((unsigned)(n_itiles * A * S)), dim3(SC_RED_THREADS), 0, s, part, cnt, lab8, n, W, (int)A, (int)S,
                       n_itiles, d_score ? d_score + i0 * A * S : nullptr, d_ne ? d_ne + i0 * A : nullptr, d_ns ? d_ns + i0 * A : nullptr,
                       d_nm ? d_nm + i0 * A : nullptr);
    GNX_HIPRET(hipGetLastError());
  }
  return hipSuccess;
}

// the _dev entry after score_check, N > 0.  *wrote: the outputs were written (GNX_OK, or GNX_EINVAL for labels out of range).
int score_dev_run(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N, int64_t C,
                  int64_t M, int64_t W, int32_t A, const double* d_weights, int32_t S, const uint8_t* d_effect, double* d_score, int32_t* d_n_effect,
                  int32_t* d_n_scored, int32_t* d_n_miss, int64_t dbg_wpb, int64_t dbg_rpp, int64_t* n_bad, bool* wrote) {
  *wrote = false;
  hipStream_t s = ctx->stream;
  int rc;
  unsigned long long* d_bad;
  if ((rc = gnx_sum_bad_counter(ctx, 3, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = score_verify(ctx, "ancestry_score", d_weights, d_effect, C, A, S, d_bad, s)) != GNX_OK) return rc;
  const int64_t rp = sc_rows_per_pass(N, W, S, dbg_rpp);
  if ((rc = score_reserve(ctx, rp, W, S)) != GNX_OK) return rc;
  HIPCHK(ctx, score_launch(ctx, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_weights, S, d_effect, d_score, d_n_effect, d_n_scored,
                           d_n_miss, dbg_wpb, rp, d_bad, s));
  unsigned long long h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *wrote = true;
  return gnx_sum_label_verdict(ctx, "ancestry_score", h_bad, A, SC_TAIL, n_bad);
}
}  // namespace

extern "C" int gnx_ancestry_score_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                      int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_weights, int32_t S,
                                      const uint8_t* d_effect, double* d_score, int32_t* d_n_effect, int32_t* d_n_scored, int32_t* d_n_miss,
                                      int64_t debug_windows_per_block, int64_t debug_rows_per_pass, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = score_check(ctx, "ancestry_score", false, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_weights, S, d_effect,
                       debug_windows_per_block, debug_rows_per_pass);
  if (rc != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  bool wrote;
  return score_dev_run(ctx, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_weights, S, d_effect, d_score, d_n_effect, d_n_scored,
                       d_n_miss, debug_windows_per_block, debug_rows_per_pass, n_bad, &wrote);
}

namespace {
// the host weights and effect -> ws_scale; the outputs' slabs in ws_b64 / ws_b32 (NULL for an output the caller did not ask for)
struct ScoreHostBufs {
  double* d_w;
  uint8_t* d_eff;
  double* d_score;
  int32_t *d_ne, *d_ns, *d_nm;
  size_t ib;   // bytes of one int32 output
};

int score_host_bufs(gnx_ctx* ctx, int64_t N, int64_t C, int32_t A, int32_t S, const double* weights, const uint8_t* effect, const void* score,
                    const void* n_effect, const void* n_scored, const void* n_miss, ScoreHostBufs* B, hipStream_t s) {
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t wb = (size_t)C * A * S * 8, ib = (size_t)(N / 2) * A * 4;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_scale, up(wb) + (size_t)C + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b64, (size_t)(N / 2) * A * S * 8 + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b32, 3 * up(ib) + 64)) != GNX_OK) return rc;
  B->d_w = (double*)ctx->ws_scale.p;
  B->d_eff = (uint8_t*)ctx->ws_scale.p + up(wb);
  B->d_score = score ? (double*)ctx->ws_b64.p : nullptr;
  char* o = (char*)ctx->ws_b32.p;
  B->d_ne = n_effect ? (int32_t*)o : nullptr;
  B->d_ns = n_scored ? (int32_t*)(o + up(ib)) : nullptr;
  B->d_nm = n_miss ? (int32_t*)(o + 2 * up(ib)) : nullptr;
  B->ib = ib;
  HIPCHK(ctx, hipMemcpyAsync(B->d_w, weights, wb, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(B->d_eff, effect, (size_t)C, hipMemcpyHostToDevice, s));
  return GNX_OK;
}

int score_copy_out(gnx_ctx* ctx, const ScoreHostBufs& B, int64_t N, int32_t A, int32_t S, double* score, int32_t* n_effect, int32_t* n_scored,
                   int32_t* n_miss, hipStream_t s) {
  if (score) HIPCHK(ctx, hipMemcpyAsync(score, B.d_score, (size_t)(N / 2) * A * S * 8, hipMemcpyDeviceToHost, s));
  if (n_effect) HIPCHK(ctx, hipMemcpyAsync(n_effect, B.d_ne, B.ib, hipMemcpyDeviceToHost, s));
  if (n_scored) HIPCHK(ctx, hipMemcpyAsync(n_scored, B.d_ns, B.ib, hipMemcpyDeviceToHost, s));
  if (n_miss) HIPCHK(ctx, hipMemcpyAsync(n_miss, B.d_nm, B.ib, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}
}  // namespace

extern "C" int gnx_ancestry_score(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                                  int64_t C, int64_t M, int64_t W, int32_t A, const double* weights, int32_t S, const uint8_t* effect, double* score,
                                  int32_t* n_effect, int32_t* n_scored, int32_t* n_miss, int64_t debug_windows_per_block,
                                  int64_t debug_rows_per_pass, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = score_check(ctx, "ancestry_score", false, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A, weights, S, effect,
                       debug_windows_per_block, debug_rows_per_pass);
  if (rc != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  ScoreHostBufs B;
  if ((rc = gnx_sum_stage_rows_labels(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  if ((rc = score_host_bufs(ctx, N, C, A, S, weights, effect, score, n_effect, n_scored, n_miss, &B, s)) != GNX_OK) return rc;
  bool wrote;
  rc = score_dev_run(ctx, ctx->ws_xu.p, row_kind, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, B.d_w, S, B.d_eff, B.d_score, B.d_ne,
                     B.d_ns, B.d_nm, debug_windows_per_block, debug_rows_per_pass, n_bad, &wrote);
  if (!wrote) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the outputs stand and are handed over)
  const std::string msg = ctx->err;
  const int rc2 = score_copy_out(ctx, B, N, A, S, score, n_effect, n_scored, n_miss, s);
  if (rc2 != GNX_OK) return rc2;
  ctx->err = msg;
  return rc;
}

// The file path's form: the packed rows of gnx_infer_gt2's batches (gnx_summary_host.h: the staging, column map, row pitch and batch
// size), scored against the caller's labels batch by batch.  A batch holds whole individuals (its size is a multiple of 4 haplotypes)
// and an individual's sums never leave its batch, so the outputs do not depend on the batch size.
extern "C" int gnx_ancestry_score_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels,
                                      const double* weights, int32_t S, const uint8_t* effect, double* score, int32_t* n_effect, int32_t* n_scored,
                                      int32_t* n_miss, int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  const char* who = "ancestry_score_gt2";
  int rc = gnx_sum_gt2_args(ctx, who, G, V, ldg, N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = score_check(ctx, who, true, nullptr, GNX_ROWS_PACKED2, (C + 3) / 4, labels, W, N, C, M, W, A, weights, S, effect, 0, 0)) != GNX_OK) return rc;
  if ((rc = gnx_sum_check_src(ctx, who, src, C, V)) != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  gnx_sum_gt2 st;
  ScoreHostBufs B;
  unsigned long long* d_bad;
  if ((rc = score_host_bufs(ctx, N, C, A, S, weights, effect, score, n_effect, n_scored, n_miss, &B, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 3, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = score_verify(ctx, who, B.d_w, B.d_eff, C, A, S, d_bad, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, true, &st, s)) != GNX_OK) return rc;
  const int64_t rp = sc_rows_per_pass(std::min(st.nb, N), W, S, 0);
  if ((rc = score_reserve(ctx, rp, W, S)) != GNX_OK) return rc;
  for (int64_t n0 = 0; n0 < N; n0 += st.nb) {   // (nb is a multiple of 4: a batch holds whole individuals)
    const int64_t n = std::min(st.nb, N - n0), i0 = n0 / 2;
    HIPCHK(ctx, gnx_sum_gt2_batch(st, n0, n, C, ctx->ws_xu.p, s));
    HIPCHK(ctx, score_launch(ctx, ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab + n0 * W, W, n, C, M, W, A, B.d_w, S, B.d_eff,
                             B.d_score ? B.d_score + i0 * A * S : nullptr, B.d_ne ? B.d_ne + i0 * A : nullptr, B.d_ns ? B.d_ns + i0 * A : nullptr,
                             B.d_nm ? B.d_nm + i0 * A : nullptr, 0, rp, d_bad, s));
  }
  unsigned long long h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  if ((rc = score_copy_out(ctx, B, N, A, S, score, n_effect, n_scored, n_miss, s)) != GNX_OK) return rc;
  return gnx_sum_label_verdict(ctx, who, h_bad, A, SC_TAIL, n_bad);
}
