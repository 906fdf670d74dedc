// summary/k_ancestry_ld.hip — ancestry-specific linkage disequilibrium on the int8 matrix cores: for ONE ancestry a, the SNPs c of a range
// [c0, c1) and the offsets 0 <= k < band, four exact int32 sums over the haplotypes h, c' = c + k:
//   n11[c, k] = sum_h d[h, c] d[h, c']    n1o[c, k] = sum_h d[h, c] o[h, c']    no1[c, k] = sum_h o[h, c] d[h, c']    noo[c, k] = sum_h o[h, c] o[h, c']
// where, with win(c) = min(c / M, W - 1),
//   o[h, c] = 1 if labels[h, win(c)] == a AND the call is observed (code 0 or 1), else 0        d[h, c] = 1 if o[h, c] and the code is 1, else 0
// Every term is 0 or 1, so int32 is exact for every N < 2^31.  The host derives r and r^2 from them (gnomix_amd/ld.py).
// This is k_ancestry_pairs.hip turned on its side: that kernel contracts over SNPs and gives individual x individual tables, this one
// contracts over haplotypes and gives SNP x SNP tables, of which only a band beside the diagonal is kept.
//
// k_ancestry_ld<KIND>: a workgroup = 256 threads = 4 waves owns a tile I of GRAM_T = 64 SNPs and a tile J >= I of 64 SNPs (tiles start at
//   multiples of 64 from t0 = c0 rounded down to 64, so a group of 16 SNPs starts at a multiple of 16), and a SEGMENT of the haplotypes,
//   which it walks in chunks of GRAM_KC = 128 (gnx_as_gram.h: the products, their operand layout, the LDS pitch's read side, the split's
//   atomics).  J is one of the (band + 62) / 64 + 1 tiles I, I + 1, ... the band of I can reach (the last SNP of I, 63, reaches
//   63 + band - 1); tiles that start at or beyond C hold nothing and are not launched (ld_geometry, ld_pair below).
//  * Fused, transposing staging.  The MFMA's K dimension is the haplotype, but a row of X is one haplotype.  An item is (4 consecutive
//    haplotypes, 16 SNPs): per haplotype one as_fields16 load and the mask of the SNPs whose window carries a (as_label_mask16), d and o
//    as ONE BIT per SNP; then per SNP the four haplotypes' bits are spread to the four bytes of one dword, which is stored to
//    image[snp][hap]: that store is the transposition.  Four images of 64 rows (d and o of I, d and o of J); a diagonal pair stages its
//    tile once and reads it for both operands.  No (N, C) intermediate exists in HBM.  Haplotypes >= N and SNPs >= C are staged as zeros,
//    which add nothing.  Nothing is read past a row's last byte (as_fields16) and a label is only compared with a, never used as an index.
//  * Products.  All four are formed on the diagonal too: the band wants [c, c'] with c' >= c of each, and O_I D_I^T is not D_I O_I^T.
//  * LDS, the store side.  The staging stores are 4 bytes wide; such a store is served in two groups of 32 consecutive lanes, banked by
//    dword address mod 32.  Items are numbered so that the 32 lanes of a group hold the 32 haplotype quads of ONE group of 16 SNPs (thread
//    t: tile t / 128, SNP group (t / 32) % 4, quad t % 32): at each of its 16 stores a group writes the dwords 0 .. 31 of one staged row, 32
//    consecutive dwords = every bank once, whatever the pitch.  The other numbering (lanes along SNPs) would put lane l at l pitch / 4
//    mod 32 = 8 l mod 32 (pitch 160): 8-way.  (The grouping is taken from public measurements of this chip; SQ_LDS_BANK_CONFLICT has not
//    been read on this kernel.)
//  * Stores.  Element (c, c') of a product goes to table[c - c0, c' - c] iff c0 <= c < c1, 0 <= c' - c < band and c' < C: the pair (I, J)
//    that holds (c, c') is unique, so every element has one owner.  Entries with c + k >= C have no owner; the host zeroes them first.
//  * The split over haplotype segments.  A short range or a small band gives few tile pairs (256 SNPs, band 64: 8 pairs for 256 CUs).  A
//    workspace plus a reduce kernel would cost segments x 4 tables written and read again; a segment is at least 4 chunks.
//  * Row reads (the known weak point, left as it is): a tile reads 16 bytes (int8) or 4 bytes (packed) per haplotype and group of 16 SNPs,
//    from rows ld_rows apart, and every J tile is staged again by each I that meets it.  DESIGN.md 4.22 says what the next step is.
// The labels outside [0, A) in the windows the range and its band reach are counted for the verdict after the launch.
// No scratch, no runtime-indexed register array, plain vector stores or vector atomics only.  Index arithmetic is 64-bit throughout.
#include "gnx_as_gram.h"

namespace {

constexpr int64_t LD_MIN_CHUNKS = 4;                   // chunks of a segment, at least (the built-in split)

struct LdLaunch {
  const uint8_t* rows;
  const int32_t* lab;
  int64_t ld, ldl, N, C, M, W, c0, c1, t0, band, cpb, ldt;   // t0: c0 rounded down to a tile; cpb: chunks per segment
  int64_t nJ, nT, full;                                      // J tiles per I at most; tiles from t0 to C; I tiles that have all nJ
  int32_t a, nseg, atomic, aligned;
  int32_t *n11, *n1o, *no1, *noo;
};

// the tile pairs of a launch: I tiles bi = 0 .. nI - 1 (those that meet [c0, c1)), each with the J tiles bi + dj, dj < nJ, that start below C
struct LdGeometry {
  int64_t t0, nI, nJ, nT, full, pairs;
};

LdGeometry ld_geometry(int64_t C, int64_t c0, int64_t c1, int64_t band) {
  LdGeometry g;
  g.t0 = c0 / GRAM_T * GRAM_T;
  g.nI = (c1 - g.t0 + GRAM_T - 1) / GRAM_T;
  g.nJ = (band + 62) / GRAM_T + 1;
  g.nT = (C - g.t0 + GRAM_T - 1) / GRAM_T;                                  // >= nI
  g.full = std::max<int64_t>(0, std::min(g.nI, g.nT - g.nJ + 1));       // I tiles bi with bi + nJ <= nT
  g.pairs = g.full * g.nJ;
  for (int64_t bi = g.full; bi < g.nI; ++bi) g.pairs += g.nT - bi;      // fewer than nJ turns
  return g;
}

// pair -> (bi, dj); the inverse of ld_geometry's count
__device__ __forceinline__ void ld_pair(const LdLaunch& L, int64_t pair, int64_t* bi, int64_t* dj) {
  if (pair < L.full * L.nJ) {
    *bi = pair / L.nJ;
    *dj = pair - *bi * L.nJ;
    return;
  }
  int64_t r = pair - L.full * L.nJ, b = L.full;
  while (r >= L.nT - b) {     // fewer than nJ turns
    r -= L.nT - b;
    ++b;
  }
  *bi = b;
  *dj = r;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_ancestry_ld(LdLaunch L) {
  __shared__ __attribute__((aligned(16))) uint8_t tz[4 * GRAM_IMG];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lq = lane >> 4;
  const uint32_t pair = blockIdx.x / (uint32_t)L.nseg, seg = blockIdx.x - pair * (uint32_t)L.nseg;
  int64_t bi, dj;
  ld_pair(L, (int64_t)pair, &bi, &dj);
  const bool diag = dj == 0;
  const int64_t iI = L.t0 + bi * GRAM_T, iJ = iI + dj * GRAM_T;                  // the tiles' first SNPs; iJ < C by the grid
  const int64_t h0 = (int64_t)seg * L.cpb * GRAM_KC;                           // < N by the grid
  const int64_t h1 = (h0 + L.cpb * GRAM_KC < L.N) ? h0 + L.cpb * GRAM_KC : L.N;

  v4i dd[4], dx[4], xd[4], oo[4];   // D_I D_J^T, D_I O_J^T, O_I D_J^T, O_I O_J^T
  gram_zero(dd, dx, xd, oo);
  const uint8_t* ap = tz + gram_a_off(wv, lr, lq);
  const uint8_t* bp = tz + gram_b_off(diag ? 0 : 2 * GRAM_IMG, lr, lq);

  // this thread's item: tile, group of 16 SNPs, quad of haplotypes
  const int tile = t >> 7, g = (t >> 5) & 3, q = t & 31;
  const int64_t cg = (tile ? iJ : iI) + 16 * g;                              // a multiple of 16
  const int64_t hi = cg + 16 < L.C ? cg + 16 : L.C;
  const bool stages = (tile == 0 || !diag) && cg < L.C;                      // (a group at or beyond C stays zero: zeroed once, below)
  uint8_t* const dst = tz + (2 * tile) * GRAM_IMG + (16 * g) * GRAM_P + 4 * q;
  if (!stages && (tile == 0 || !diag)) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      *reinterpret_cast<uint32_t*>(dst + j * GRAM_P) = 0u;
      *reinterpret_cast<uint32_t*>(dst + GRAM_IMG + j * GRAM_P) = 0u;
    }
  }

  for (int64_t k0 = h0; k0 < h1; k0 += GRAM_KC) {
    if (stages) {
      uint32_t d01 = 0, d23 = 0, o01 = 0, o23 = 0;      // bits 2 j, 2 j + 1 = SNP j of the quad's haplotypes 0, 1 (2, 3)
#pragma unroll
      for (int hq = 0; hq < 4; ++hq) {
        const int64_t h = k0 + 4 * q + hq;
        uint32_t db = 0, ob = 0;
        if (h < h1) {
          uint32_t obs, alt;
          as_obs_alt(as_fields16<KIND>(L.rows + h * L.ld, cg, L.C, L.aligned), &obs, &alt);
          const uint32_t m = as_label_mask16(L.lab + h * L.ldl, L.a, cg, cg, hi, L.C, L.M, L.W);
          db = alt & m;
          ob = obs & m;
        }
        if (hq == 0) { d01 = db; o01 = ob; }
        else if (hq == 1) { d01 |= db << 1; o01 |= ob << 1; }
        else if (hq == 2) { d23 = db; o23 = ob; }
        else { d23 |= db << 1; o23 |= ob << 1; }
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        // bits 0, 1, 16, 17 = the four haplotypes; bit 1 -> 8 and bit 17 -> 24 by the shift of 7
        uint32_t wd = ((d01 >> (2 * j)) & 3u) | (((d23 >> (2 * j)) & 3u) << 16);
        uint32_t wo = ((o01 >> (2 * j)) & 3u) | (((o23 >> (2 * j)) & 3u) << 16);
        wd = (wd | (wd << 7)) & 0x01010101u;
        wo = (wo | (wo << 7)) & 0x01010101u;
        *reinterpret_cast<uint32_t*>(dst + j * GRAM_P) = wd;
        *reinterpret_cast<uint32_t*>(dst + GRAM_IMG + j * GRAM_P) = wo;
      }
    }
    __syncthreads();
    gram_chunk(ap, bp, true, dd, dx, xd, oo);
    __syncthreads();
  }

  const size_t ldt = (size_t)L.ldt;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t c = gram_row(iI, wv, lq, r);
      const int64_t c2 = gram_col(iJ, lr, jt);
      const int64_t k = c2 - c;
      if (c < L.c0 || c >= L.c1 || k < 0 || k >= L.band || c2 >= L.C) continue;
      const size_t at = (size_t)(c - L.c0) * ldt + (size_t)k;
      if (L.n11) gram_put(L.n11, at, dd[jt][r], L.atomic);
      if (L.n1o) gram_put(L.n1o, at, dx[jt][r], L.atomic);
      if (L.no1) gram_put(L.no1, at, xd[jt][r], L.atomic);
      if (L.noo) gram_put(L.noo, at, oo[jt][r], L.atomic);
    }
}

// the op the three forms run: (c1 - c0) x band tables n11, n1o, no1, noo
struct LdOp {
  gnx_gram_call c;
  int64_t band;
  LdOp(const char* who, int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11,
       int32_t* n1o, int32_t* no1, int32_t* noo, int64_t ld, int64_t* n_bad)
      : c{who, N, C, M, W, A, ancestry, c0, c1, 4, {n11, n1o, no1, noo}, ld, c1 - c0, band, n_bad}, band(band) {}

  int check(gnx_ctx* ctx, bool built, const gnx_gram_rows& R, int64_t dbg) const {
    const std::string w(c.who);
    int rc = gnx_gram_check_range(ctx, c, built ? GNX_SUM_ROWS_BUILT : 0u, R);
    if (rc != GNX_OK) return rc;
    if (band < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": band must be >= 1");
    if (c.ld < band) return gnx_fail(ctx, GNX_EINVAL, w + ": the tables' row stride is smaller than band");
    if ((rc = gnx_gram_check_sizes(ctx, c, dbg)) != GNX_OK) return rc;
    if (band > GNX_LD_MAX_BAND) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": band = " + std::to_string(band) + ", at most " + std::to_string(GNX_LD_MAX_BAND));
    return GNX_OK;
  }

  int run(gnx_ctx* ctx, const gnx_gram_rows& R, int32_t* const tabs[], int64_t ld, int64_t dbg, unsigned long long* d_bad, hipStream_t s) const {
    const int64_t N = c.N, C = c.C, c0 = c.c0, c1 = c.c1;
    const LdGeometry g = ld_geometry(C, c0, c1, band);
    int64_t cpb, nseg;
    gnx_gram_split((N + GRAM_KC - 1) / GRAM_KC, g.pairs, ctx->n_cu, dbg, LD_MIN_CHUNKS, &cpb, &nseg);
    int rc = gnx_gram_grid_check(ctx, c.who, g.pairs, nseg, "haplotype");
    if (rc != GNX_OK) return rc;
    const int64_t last = std::min(c1 - 1 + band - 1, C - 1);     // the last SNP the band reaches
    if ((rc = gnx_gram_count_labels(ctx, R.labels, R.ld_labels, N, as_win(c0, c.M, c.W), as_win(last, c.M, c.W) + 1, c.A, d_bad, s)) != GNX_OK) return rc;
    if (!tabs[0] && !tabs[1] && !tabs[2] && !tabs[3]) return GNX_OK;
    const int atomic = nseg > 1;
    // zeroed first: everything where the segments add; else the rows whose band reaches beyond C (those entries have no owner)
    const int64_t z0 = atomic ? 0 : std::max(c0, C - band + 1) - c0;
    if (z0 < c1 - c0 && (rc = gnx_gram_zero(ctx, tabs, 4, ld, z0, c1 - c0 - z0, band, s)) != GNX_OK) return rc;
    const int aligned = gnx_sum_rows_aligned(R.rows, R.row_kind, R.ld_rows);
    LdLaunch L{(const uint8_t*)R.rows, R.labels, R.ld_rows, R.ld_labels, N, C, c.M, c.W, c0, c1, g.t0, band, cpb, ld, g.nJ, g.nT, g.full,
               c.ancestry, (int32_t)nseg, atomic, aligned, tabs[0], tabs[1], tabs[2], tabs[3]};
    const dim3 grid((unsigned)(g.pairs * nseg));
    if (R.row_kind == GNX_ROWS_PACKED2) hipLaunchKernelGGL(k_ancestry_ld<GNX_ROWS_PACKED2>, grid, dim3(256), 0, s, L);
    else hipLaunchKernelGGL(k_ancestry_ld<GNX_ROWS_INT8>, grid, dim3(256), 0, s, L);
    HIPCHK(ctx, hipGetLastError());
    return GNX_OK;
  }
};

}  // namespace

extern "C" int gnx_ancestry_ld_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                          int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band,
                                          int32_t* d_n11, int32_t* d_n1o, int32_t* d_no1, int32_t* d_noo, int64_t ld, int64_t debug_haps_per_block,
                                          int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const LdOp op("ancestry_ld_counts", N, C, M, W, A, ancestry, c0, c1, band, d_n11, d_n1o, d_no1, d_noo, ld, n_bad);
  return gnx_gram_form_dev(ctx, op, gnx_gram_rows{d_rows, row_kind, ld_rows, d_labels, ld_labels}, debug_haps_per_block);
}

extern "C" int gnx_ancestry_ld_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                                      int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11,
                                      int32_t* n1o, int32_t* no1, int32_t* noo, int64_t ld, int64_t debug_haps_per_block, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const LdOp op("ancestry_ld_counts", N, C, M, W, A, ancestry, c0, c1, band, n11, n1o, no1, noo, ld, n_bad);
  return gnx_gram_form_host(ctx, op, gnx_gram_rows{rows, row_kind, ld_rows, labels, ld_labels}, debug_haps_per_block);
}

extern "C" int gnx_ancestry_ld_counts_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels,
                                          int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11, int32_t* n1o, int32_t* no1, int32_t* noo,
                                          int64_t ld, int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  const LdOp op("ancestry_ld_counts_gt2", N, m->info.C, m->info.M, m->info.W, m->info.A, ancestry, c0, c1, band, n11, n1o, no1, noo, ld, n_bad);
  return gnx_gram_form_gt2(m->ctx, op, G, V, ldg, src, labels);
}
