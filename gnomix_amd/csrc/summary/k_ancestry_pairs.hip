// summary/k_ancestry_pairs.hip — ancestry-specific pairwise counts on the int8 matrix cores: for ONE ancestry a and every pair of
// individuals (i, j), three exact int32 sums over the SNPs c of a range [c0, c1),
//   DD[i, j] = sum_c d[i, c] d[j, c]   (symmetric)     DO[i, j] = sum_c d[i, c] o[j, c]   (NOT symmetric)     OO[i, j] = sum_c o[i, c] o[j, c]
// where, with individual i = haplotype rows 2 i, 2 i + 1 and win(c) = min(c / M, W - 1),
//   o[i, c] = how many of the two haplotypes h have labels[h, win(c)] == a AND an observed call (code 0 or 1)      0..2
//   d[i, c] = how many of those have code 1                                                                       0..o
// (o is NOT k_allele_counts.hip's hapcount, which also counts missing calls).  Every term is in 0..4, so int32 is exact while
// 4 (c1 - c0) < 2^31 (refused beyond).  The host derives the mismatching and the compared haplotype pairs from them (gnomix_amd/asmds.py).
//
// k_ancestry_pairs<KIND>: a workgroup = 256 threads = 4 waves owns a pair (I, J), I >= J, of tiles of GRAM_T = 64 individuals and a
//   SEGMENT of the SNP range, which it walks in chunks of GRAM_KC = 128 SNPs that start at multiples of GRAM_KC (gnx_as_gram.h: the
//   products, their operand layout, the LDS pitch's read side, the split's atomics).
//  * Fused staging.  Per chunk the INDIVIDUAL-level bytes d and o of both tiles go to LDS (four images of 64 rows); an item is one
//    (individual, 16 SNPs): the two haplotypes' 16 fields (as_fields16: one load per haplotype for either row form), the mask of the SNPs
//    whose window carries label a (as_label_mask16), d and o as 2-bit fields by two adds, widened to bytes by shifts, two 16-byte stores.
//    No (N, C) intermediate exists in HBM.  Individuals >= n and SNPs outside [c0, c1) are staged as zeros, which add nothing: that is
//    how partial tiles, partial chunks and ranges that start or end anywhere are made safe.  Nothing is read past a row's last byte
//    (as_fields16) and a label is only compared with a, never used as an index.
//  * LDS, the store side.  The 16-byte stores of an item go out in groups of 8 consecutive lanes = the 8 items of one row = 128
//    consecutive bytes: conflict-free under the pitch of 160 bytes as well.
//  * Products and stores.  On a diagonal pair (I == J) the tile's own products hold both halves, so O_I D_J^T is not formed and the
//    64 x 64 tiles are stored as they are.  Off the diagonal a workgroup stores DD[I, J] and OO[I, J] with their mirror images, DO[I, J] =
//    D_I O_J^T and DO[J, I] = (O_I D_J^T)^T.  So no element has two owners.
//  * The split over SNP segments.  With few individuals the pairs alone do not fill the chip (n = 200: ten pairs for 256 CUs).  A
//    workspace plus a reduce kernel would cost segments x 3 n^2 x 4 bytes written and read again; a segment is at least 8 chunks.  One
//    segment (the case of many individuals) uses plain stores and zeroes nothing.
// The labels outside [0, A) in the windows that meet [c0, c1) are counted for the verdict after the launch.
// No scratch, no runtime-indexed register array, plain vector stores or vector atomics only.  Index arithmetic is 64-bit throughout.
#include "gnx_as_gram.h"

namespace {

constexpr int PR_G = GRAM_KC / 16;                     // groups of 16 SNPs per chunk
constexpr int PR_ITEMS = 2 * GRAM_T * PR_G / 256;      // (individual, group) items per thread and chunk
constexpr int64_t PR_MIN_CHUNKS = 8;                   // chunks of a segment, at least (the built-in split)

struct PairsLaunch {
  const uint8_t* rows;
  const int32_t* lab;
  int64_t ld, ldl, n, C, M, W, c0, c1, t0, cpb, ldt;   // n individuals; t0: c0 rounded down to a chunk; cpb: chunks per segment
  int32_t a, nseg, atomic, aligned;
  int32_t *DD, *DO, *OO;
};

// four 2-bit fields (bits 0..7 of x) -> four bytes
__device__ __forceinline__ uint32_t pr_widen(uint32_t x) { return (x | (x << 6) | (x << 12) | (x << 18)) & 0x03030303u; }

template <int KIND>
__global__ __launch_bounds__(256) void k_ancestry_pairs(PairsLaunch L) {
  __shared__ __attribute__((aligned(16))) uint8_t tz[4 * GRAM_IMG];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lq = lane >> 4;
  const uint32_t pair = blockIdx.x / (uint32_t)L.nseg, seg = blockIdx.x - pair * (uint32_t)L.nseg;
  // pair -> (bi, bj), bi >= bj: bi (bi + 1) / 2 + bj
  int64_t bi = (int64_t)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= (int64_t)pair) ++bi;
  while (bi * (bi + 1) / 2 > (int64_t)pair) --bi;
  const int64_t bj = (int64_t)pair - bi * (bi + 1) / 2;
  const bool diag = bi == bj;
  const int64_t s0 = L.t0 + (int64_t)seg * L.cpb * GRAM_KC;                  // a multiple of GRAM_KC, < c1 by the grid
  const int64_t s1 = (s0 + L.cpb * GRAM_KC < L.c1) ? s0 + L.cpb * GRAM_KC : L.c1;

  v4i dd[4], dx[4], xd[4], oo[4];   // D_I D_J^T, D_I O_J^T, O_I D_J^T, O_I O_J^T
  gram_zero(dd, dx, xd, oo);
  const uint8_t* ap = tz + gram_a_off(wv, lr, lq);
  const uint8_t* bp = tz + gram_b_off(2 * GRAM_IMG, lr, lq);

  for (int64_t k0 = s0; k0 < s1; k0 += GRAM_KC) {
#pragma unroll
    for (int it = 0; it < PR_ITEMS; ++it) {
      const int idx = t + 256 * it;
      const int tile = idx / (GRAM_T * PR_G), r = (idx / PR_G) % GRAM_T, g = idx % PR_G;
      const int64_t ind = (tile ? bj : bi) * GRAM_T + r, cg = k0 + 16 * g;
      const int64_t lo = cg > L.c0 ? cg : L.c0, hi = cg + 16 < s1 ? cg + 16 : s1;
      uint32_t dw = 0, ow = 0;      // d and o of the 16 SNPs as 2-bit fields
      if (ind < L.n && lo < hi) {
#pragma unroll
        for (int hap = 0; hap < 2; ++hap) {
          const int64_t h = 2 * ind + hap;
          uint32_t obs, alt;
          as_obs_alt(as_fields16<KIND>(L.rows + h * L.ld, cg, L.C, L.aligned), &obs, &alt);
          const uint32_t m = as_label_mask16(L.lab + h * L.ldl, L.a, cg, lo, hi, L.C, L.M, L.W);
          dw += alt & m;
          ow += obs & m;
        }
      }
      uint8_t* dst = tz + (2 * tile) * GRAM_IMG + r * GRAM_P + 16 * g;
      *reinterpret_cast<uint4*>(dst) = uint4{pr_widen(dw & 0xFFu), pr_widen((dw >> 8) & 0xFFu), pr_widen((dw >> 16) & 0xFFu), pr_widen(dw >> 24)};
      *reinterpret_cast<uint4*>(dst + GRAM_IMG) = uint4{pr_widen(ow & 0xFFu), pr_widen((ow >> 8) & 0xFFu), pr_widen((ow >> 16) & 0xFFu), pr_widen(ow >> 24)};
    }
    __syncthreads();
    gram_chunk(ap, bp, !diag, dd, dx, xd, oo);
    __syncthreads();
  }

  const size_t ldt = (size_t)L.ldt;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = gram_row(bi * GRAM_T, wv, lq, r);
      const int64_t j = gram_col(bj * GRAM_T, lr, jt);
      if (i >= L.n || j >= L.n) continue;
      const size_t ij = (size_t)i * ldt + (size_t)j, ji = (size_t)j * ldt + (size_t)i;
      if (L.DD) gram_put(L.DD, ij, dd[jt][r], L.atomic);
      if (L.OO) gram_put(L.OO, ij, oo[jt][r], L.atomic);
      if (L.DO) gram_put(L.DO, ij, dx[jt][r], L.atomic);
      if (!diag) {
        if (L.DD) gram_put(L.DD, ji, dd[jt][r], L.atomic);
        if (L.OO) gram_put(L.OO, ji, oo[jt][r], L.atomic);
        if (L.DO) gram_put(L.DO, ji, xd[jt][r], L.atomic);
      }
    }
}

// the op the three forms run: n x n tables DD, DO, OO, n = N / 2
struct PairsOp {
  gnx_gram_call c;
  PairsOp(const char* who, int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO,
          int32_t* OO, int64_t ld, int64_t* n_bad)
      : c{who, N, C, M, W, A, ancestry, c0, c1, 3, {DD, DO, OO, nullptr}, ld, N / 2, N / 2, n_bad} {}

  int check(gnx_ctx* ctx, bool built, const gnx_gram_rows& R, int64_t dbg) const {
    const std::string w(c.who);
    int rc = gnx_gram_check_range(ctx, c, GNX_SUM_N_EVEN | (built ? GNX_SUM_ROWS_BUILT : 0u), R);
    if (rc != GNX_OK) return rc;
    if (c.ld < c.N / 2) return gnx_fail(ctx, GNX_EINVAL, w + ": the tables' row stride is smaller than N / 2");
    if ((rc = gnx_gram_check_sizes(ctx, c, dbg)) != GNX_OK) return rc;
    if (c.c1 - c.c0 >= ((int64_t)1 << 29)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": c1 - c0 must be below 2^29 (a sum of terms up to 4 is int32)");
    return GNX_OK;
  }

  int run(gnx_ctx* ctx, const gnx_gram_rows& R, int32_t* const tabs[], int64_t ld, int64_t dbg, unsigned long long* d_bad, hipStream_t s) const {
    const int64_t n = c.N / 2, T = (n + GRAM_T - 1) / GRAM_T, pairs = T * (T + 1) / 2, t0 = c.c0 / GRAM_KC * GRAM_KC;
    int64_t cpb, nseg;
    gnx_gram_split((c.c1 - t0 + GRAM_KC - 1) / GRAM_KC, pairs, ctx->n_cu, dbg, PR_MIN_CHUNKS, &cpb, &nseg);
    int rc = gnx_gram_grid_check(ctx, c.who, pairs, nseg, "SNP");
    if (rc != GNX_OK) return rc;
    if ((rc = gnx_gram_count_labels(ctx, R.labels, R.ld_labels, c.N, as_win(c.c0, c.M, c.W), as_win(c.c1 - 1, c.M, c.W) + 1, c.A, d_bad, s)) != GNX_OK)
      return rc;
    if (!tabs[0] && !tabs[1] && !tabs[2]) return GNX_OK;
    const int atomic = nseg > 1;   // zeroed first: everything, where the segments add
    if (atomic && (rc = gnx_gram_zero(ctx, tabs, 3, ld, 0, n, n, s)) != GNX_OK) return rc;
    const int aligned = gnx_sum_rows_aligned(R.rows, R.row_kind, R.ld_rows);
    PairsLaunch L{(const uint8_t*)R.rows, R.labels, R.ld_rows, R.ld_labels, n, c.C, c.M, c.W, c.c0, c.c1, t0, cpb, ld,
                  c.ancestry, (int32_t)nseg, atomic, aligned, tabs[0], tabs[1], tabs[2]};
    const dim3 grid((unsigned)(pairs * nseg));
    if (R.row_kind == GNX_ROWS_PACKED2) hipLaunchKernelGGL(k_ancestry_pairs<GNX_ROWS_PACKED2>, grid, dim3(256), 0, s, L);
    else hipLaunchKernelGGL(k_ancestry_pairs<GNX_ROWS_INT8>, grid, dim3(256), 0, s, L);
    HIPCHK(ctx, hipGetLastError());
    return GNX_OK;
  }
};

}  // namespace

extern "C" int gnx_ancestry_pair_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                            int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1,
                                            int32_t* d_DD, int32_t* d_DO, int32_t* d_OO, int64_t ld, int64_t debug_snps_per_block, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const PairsOp op("ancestry_pair_counts", N, C, M, W, A, ancestry, c0, c1, d_DD, d_DO, d_OO, ld, n_bad);
  return gnx_gram_form_dev(ctx, op, gnx_gram_rows{d_rows, row_kind, ld_rows, d_labels, ld_labels}, debug_snps_per_block);
}

extern "C" int gnx_ancestry_pair_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                                        int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO,
                                        int32_t* OO, int64_t ld, int64_t debug_snps_per_block, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const PairsOp op("ancestry_pair_counts", N, C, M, W, A, ancestry, c0, c1, DD, DO, OO, ld, n_bad);
  return gnx_gram_form_host(ctx, op, gnx_gram_rows{rows, row_kind, ld_rows, labels, ld_labels}, debug_snps_per_block);
}

extern "C" int gnx_ancestry_pair_counts_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels,
                                            int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO, int32_t* OO, int64_t ld,
                                            int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  const PairsOp op("ancestry_pair_counts_gt2", N, m->info.C, m->info.M, m->info.W, m->info.A, ancestry, c0, c1, DD, DO, OO, ld, n_bad);
  return gnx_gram_form_gt2(m->ctx, op, G, V, ldg, src, labels);
}
