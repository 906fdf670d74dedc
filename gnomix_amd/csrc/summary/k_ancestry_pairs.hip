// summary/k_ancestry_pairs.hip — ancestry-specific pairwise counts on the int8 matrix cores: for ONE ancestry a and every pair of
// individuals (i, j), three exact int32 sums over the SNPs c of a range [c0, c1),
//   DD[i, j] = sum_c d[i, c] d[j, c]   (symmetric)     DO[i, j] = sum_c d[i, c] o[j, c]   (NOT symmetric)     OO[i, j] = sum_c o[i, c] o[j, c]
// where, with individual i = haplotype rows 2 i, 2 i + 1 and win(c) = min(c / M, W - 1),
//   o[i, c] = how many of the two haplotypes h have labels[h, win(c)] == a AND an observed call (code 0 or 1)      0..2
//   d[i, c] = how many of those have code 1                                                                       0..o
// (o is NOT k_allele_counts.hip's hapcount, which also counts missing calls).  Every term is in 0..4, so int32 is exact while
// 4 (c1 - c0) < 2^31 (refused beyond).  The host derives the mismatching and the compared haplotype pairs from them (gnomix_amd/asmds.py).
//
// k_ancestry_pairs<KIND>: a workgroup = 256 threads = 4 waves owns a pair (I, J), I >= J, of tiles of PR_T = 64 individuals and a SEGMENT
//   of the SNP range, which it walks in chunks of PR_KC = 128 SNPs that start at multiples of PR_KC.
//  * Fused staging.  Per chunk the INDIVIDUAL-level bytes d and o of both tiles go to LDS (four images of 64 rows); an item is one
//    (individual, 16 SNPs): the two haplotypes' 16 fields (as_fields16: one load per haplotype for either row form), the mask of the SNPs
//    whose window carries label a (a loop over the windows that meet the 16 SNPs: one turn unless a boundary falls inside, 16 turns at
//    M = 1; the last window takes the remainder), d and o as 2-bit fields by two adds, widened to bytes by shifts, two 16-byte stores.
//    No (N, C) intermediate exists in HBM.  Individuals >= n and SNPs outside [c0, c1) are staged as zeros, which add nothing: that is
//    how partial tiles, partial chunks and ranges that start or end anywhere are made safe.  Nothing is read past a row's last byte
//    (as_fields16) and a label is only compared with a, never used as an index.
//  * Products.  Wave v owns rows 16 v .. 16 v + 15 of tile I and all four 16-column tiles of J: D_I D_J^T, D_I O_J^T, O_I D_J^T and
//    O_I O_J^T, 16 accumulators of four int32 each, two v_mfma_i32_16x16x64_i8 steps per chunk.  The reduction index is the SNP and X is
//    contiguous along SNPs, so both operands are 16 consecutive bytes of a staged row (A: row = lane & 15 of the wave's rows, B: row =
//    lane & 15 of the column tile, k-block = lane >> 4), the layout of k_lda_gram and k_knn_argmin; C/D: column = lane & 15, row =
//    4 (lane >> 4) + reg.  On a diagonal pair (I == J) the tile's own products hold both halves, so O_I D_J^T is not formed.
//  * LDS pitch 160 bytes (PR_KC + 32).  The hardware serves a 16-byte read of a wave in four groups of 16 lanes, and a group is not 16
//    consecutive lanes: it holds every row r = lane & 15 once, the rows 0-3 and 12-15 with one k-block q and the rows 4-11 with q + 1
//    (or the other way round).  In units of the 16-byte slot, 16 of which make the 64 banks, row r and k-block q sit at 10 r + q: 10 r
//    mod 16 = 2 (5 r mod 8) takes each even value twice, for r and r + 8, and exactly one of r and r + 8 lies in 4..11, so the + 1 of
//    that one makes the 16 slots of a group distinct: conflict-free, for both k-steps (+ 4 slots for all lanes).  An 80-byte pitch
//    (slot 5 r + q) is conflict-free only if a group were 16 consecutive lanes.  The 16-byte stores of an item go out in groups of 8
//    consecutive lanes = the 8 items of one row = 128 consecutive bytes: conflict-free as well.  (The grouping is taken from measurements
//    of this chip that are public; the counter SQ_LDS_BANK_CONFLICT on this kernel has not been read.)
//  * Stores.  Off the diagonal a workgroup stores DD[I, J] and OO[I, J] with their mirror images, DO[I, J] = D_I O_J^T and DO[J, I] =
//    (O_I D_J^T)^T; on the diagonal it stores its 64 x 64 tiles as they are, so no element has two owners.
//  * The split over SNP segments.  With few individuals the pairs alone do not fill the chip (n = 200: ten pairs for 256 CUs), so the
//    range is cut into segments of whole chunks and grid = pairs x segments.  The segments' sums are combined with int32 vector atomic adds
//    (global_atomic_add, no return value) into tables zeroed first: integer addition is associative, so the order cannot change a sum.
//    Chosen over a workspace plus a reduce kernel because that costs segments x 3 n^2 x 4 bytes written and read again and one more
//    launch, where the atomics touch each element once per segment, and a segment is at least 8 chunks of MFMA work per element.  One
//    segment (the case of many individuals) uses plain stores and zeroes nothing.
// k_ancestry_pairs_labels: the labels outside [0, A) in the windows that meet [c0, c1), counted for the verdict after the launch.
// No scratch, no runtime-indexed register array, plain vector stores or vector atomics only.  Index arithmetic is 64-bit throughout.
#include "gnx_summary_host.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int PR_T = 64;                               // individuals per tile
constexpr int PR_KC = 128;                             // SNPs per chunk: two steps of the MFMA's K = 64
constexpr int PR_P = PR_KC + 32;                       // LDS row pitch, bytes
constexpr int PR_G = PR_KC / 16;                       // groups of 16 SNPs per chunk
constexpr int PR_ITEMS = 2 * PR_T * PR_G / 256;        // (individual, group) items per thread and chunk
constexpr int PR_IMG = PR_T * PR_P;                    // bytes of one staged image
constexpr int64_t PR_MIN_CHUNKS = 8;                   // chunks of a segment, at least (the built-in split)
constexpr uint32_t PR_EVEN = 0x55555555u;

struct PairsLaunch {
  const uint8_t* rows;
  const int32_t* lab;
  int64_t ld, ldl, n, C, M, W, c0, c1, t0, cpb, ldt;   // n individuals; t0: c0 rounded down to a chunk; cpb: chunks per segment
  int32_t a, nseg, atomic, aligned;
  int32_t *DD, *DO, *OO;
};

// four 2-bit fields (bits 0..7 of x) -> four bytes
__device__ __forceinline__ uint32_t pr_widen(uint32_t x) { return (x | (x << 6) | (x << 12) | (x << 18)) & 0x03030303u; }

__device__ __forceinline__ void pr_put(int32_t* __restrict__ T, size_t at, int32_t v, int atomic) {
  if (atomic) atomicAdd(T + at, v);
  else T[at] = v;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_ancestry_pairs(PairsLaunch L) {
  __shared__ __attribute__((aligned(16))) uint8_t tz[4 * PR_IMG];  // d of tile I, o of tile I, d of tile J, o of tile J
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t pair = blockIdx.x / (uint32_t)L.nseg, seg = blockIdx.x - pair * (uint32_t)L.nseg;
  // pair -> (bi, bj), bi >= bj: bi (bi + 1) / 2 + bj
  int64_t bi = (int64_t)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= (int64_t)pair) ++bi;
  while (bi * (bi + 1) / 2 > (int64_t)pair) --bi;
  const int64_t bj = (int64_t)pair - bi * (bi + 1) / 2;
  const bool diag = bi == bj;
  const int64_t s0 = L.t0 + (int64_t)seg * L.cpb * PR_KC;                    // a multiple of PR_KC, < c1 by the grid
  const int64_t s1 = (s0 + L.cpb * PR_KC < L.c1) ? s0 + L.cpb * PR_KC : L.c1;

  v4i dd[4], dx[4], xd[4], oo[4];   // D_I D_J^T, D_I O_J^T, O_I D_J^T, O_I O_J^T
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) dd[jt] = dx[jt] = xd[jt] = oo[jt] = v4i{0, 0, 0, 0};
  const uint8_t* ap = tz + (wv * 16 + (lane & 15)) * PR_P + (lane >> 4) * 16;
  const uint8_t* bp = tz + 2 * PR_IMG + (lane & 15) * PR_P + (lane >> 4) * 16;

  for (int64_t k0 = s0; k0 < s1; k0 += PR_KC) {
#pragma unroll
    for (int it = 0; it < PR_ITEMS; ++it) {
      const int idx = t + 256 * it;
      const int tile = idx / (PR_T * PR_G), r = (idx / PR_G) % PR_T, g = idx % PR_G;
      const int64_t ind = (tile ? bj : bi) * PR_T + r, cg = k0 + 16 * g;
      const int64_t lo = cg > L.c0 ? cg : L.c0, hi = cg + 16 < s1 ? cg + 16 : s1;
      uint32_t dw = 0, ow = 0;      // d and o of the 16 SNPs as 2-bit fields
      if (ind < L.n && lo < hi) {
#pragma unroll
        for (int hap = 0; hap < 2; ++hap) {
          const int64_t h = 2 * ind + hap;
          const uint32_t f = as_fields16<KIND>(L.rows + h * L.ld, cg, L.C, L.aligned);
          const uint32_t obs = ~(f >> 1) & PR_EVEN, alt = f & obs;
          const int32_t* lh = L.lab + h * L.ldl;
          uint32_t m = 0;
          int64_t c = lo, k = lo / L.M;
          if (k > L.W - 1) k = L.W - 1;
          while (c < hi) {          // the SNPs [c, se) lie in window k
            const int64_t wend = (k == L.W - 1) ? L.C : (k + 1) * L.M;
            const int64_t se = hi < wend ? hi : wend;
            if (lh[k] == L.a) m |= as_range16((int)(c - cg), (int)(se - cg));
            c = se;
            ++k;
          }
          dw += alt & m;
          ow += obs & m;
        }
      }
      uint8_t* dst = tz + (2 * tile) * PR_IMG + r * PR_P + 16 * g;
      *reinterpret_cast<uint4*>(dst) = uint4{pr_widen(dw & 0xFFu), pr_widen((dw >> 8) & 0xFFu), pr_widen((dw >> 16) & 0xFFu), pr_widen(dw >> 24)};
      *reinterpret_cast<uint4*>(dst + PR_IMG) = uint4{pr_widen(ow & 0xFFu), pr_widen((ow >> 8) & 0xFFu), pr_widen((ow >> 16) & 0xFFu), pr_widen(ow >> 24)};
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < PR_KC / 64; ++ks) {
      const v4i ad = *reinterpret_cast<const v4i*>(ap + 64 * ks);
      const v4i ao = *reinterpret_cast<const v4i*>(ap + PR_IMG + 64 * ks);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const v4i bd = *reinterpret_cast<const v4i*>(bp + jt * 16 * PR_P + 64 * ks);
        const v4i bo = *reinterpret_cast<const v4i*>(bp + PR_IMG + jt * 16 * PR_P + 64 * ks);
        dd[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bd, dd[jt], 0, 0, 0);
        dx[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bo, dx[jt], 0, 0, 0);
        oo[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bo, oo[jt], 0, 0, 0);
        if (!diag) xd[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bd, xd[jt], 0, 0, 0);   // (block-uniform)
      }
    }
    __syncthreads();
  }

  const size_t ldt = (size_t)L.ldt;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = bi * PR_T + wv * 16 + 4 * (lane >> 4) + r;
      const int64_t j = bj * PR_T + jt * 16 + (lane & 15);
      if (i >= L.n || j >= L.n) continue;
      const size_t ij = (size_t)i * ldt + (size_t)j, ji = (size_t)j * ldt + (size_t)i;
      if (L.DD) pr_put(L.DD, ij, dd[jt][r], L.atomic);
      if (L.OO) pr_put(L.OO, ij, oo[jt][r], L.atomic);
      if (L.DO) pr_put(L.DO, ij, dx[jt][r], L.atomic);
      if (!diag) {
        if (L.DD) pr_put(L.DD, ji, dd[jt][r], L.atomic);
        if (L.OO) pr_put(L.OO, ji, oo[jt][r], L.atomic);
        if (L.DO) pr_put(L.DO, ji, xd[jt][r], L.atomic);
      }
    }
}

// labels outside [0, A) among the rows' windows [k0, k1)
__global__ __launch_bounds__(256) void k_ancestry_pairs_labels(const int32_t* __restrict__ lab, int64_t ldl, int64_t N, int64_t k0, int64_t k1, int A,
                                                               unsigned long long* __restrict__ bad) {
  const int64_t nk = k1 - k0, total = N * nk;
  unsigned int mine = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t h = e / nk, k = k0 + (e - h * nk);
    const int32_t v = lab[h * ldl + k];
    if (v < 0 || v >= A) ++mine;
  }
  if (mine) atomicAdd(bad, (unsigned long long)mine);
}

const char* const PR_TAIL = "such a haplotype counts for no ancestry at that window";

// every refusal that needs no device memory; GNX_OK or the code.  built: the rows are built by this call (the file path's form)
int pairs_check(gnx_ctx* ctx, const char* who, bool built, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels,
                int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t ld, int64_t dbg) {
  const std::string w(who);
  const int rc = gnx_sum_geometry_check(ctx, who, GNX_SUM_N_EVEN | (built ? GNX_SUM_ROWS_BUILT : 0u), rows, row_kind, ld_rows, labels, ld_labels, N, C, M,
                                        W, A);
  if (rc != GNX_OK) return rc;
  if (ancestry < 0 || ancestry >= A) return gnx_fail(ctx, GNX_EINVAL, w + ": ancestry outside [0, A)");
  if (c0 < 0 || c1 <= c0 || c1 > C) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= c0 < c1 <= C");
  if (ld < N / 2) return gnx_fail(ctx, GNX_EINVAL, w + ": the tables' row stride is smaller than N / 2");
  if (N >= ((int64_t)1 << 31)) return gnx_fail(ctx, GNX_EINVAL, w + ": N must be below 2^31");
  if (dbg < 0) return gnx_fail(ctx, GNX_EINVAL, w + ": the debug argument must be >= 0 (0 = the built-in choice)");
  if (A > GNX_ALLELE_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, at most " + std::to_string(GNX_ALLELE_MAX_A));
  if (c1 - c0 >= ((int64_t)1 << 29)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": c1 - c0 must be below 2^29 (a sum of terms up to 4 is int32)");
  return GNX_OK;
}

// the split of [c0, c1): chunks per segment and the number of segments, a function of (n, c0, c1, n_cu, dbg) alone
void pairs_split(int64_t n, int64_t c0, int64_t c1, int n_cu, int64_t dbg, int64_t* cpb, int64_t* nseg) {
  const int64_t T = (n + PR_T - 1) / PR_T, pairs = T * (T + 1) / 2;
  const int64_t t0 = c0 / PR_KC * PR_KC, chunks = (c1 - t0 + PR_KC - 1) / PR_KC;
  int64_t per = chunks;
  if (dbg > 0) {
    per = (dbg + PR_KC - 1) / PR_KC;
  } else {
    const int64_t want = (int64_t)n_cu * 4;            // about four workgroups per CU
    if (pairs < want) {
      const int64_t ns = (want + pairs - 1) / pairs;   // segments that would fill the chip
      per = std::max(PR_MIN_CHUNKS, (chunks + ns - 1) / ns);
    }
  }
  per = std::min(per, chunks);
  *cpb = per;
  *nseg = (chunks + per - 1) / per;
}

// the tables of N > 0 rows (device pointers, any table may be NULL), and the labels out of range ADDED to *d_bad.  Arguments checked.
int pairs_run(gnx_ctx* ctx, const char* who, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N,
              int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int32_t* d_DD, int32_t* d_DO, int32_t* d_OO,
              int64_t ld, int64_t dbg, unsigned long long* d_bad, hipStream_t s) {
  const int64_t n = N / 2, T = (n + PR_T - 1) / PR_T, pairs = T * (T + 1) / 2;
  int64_t cpb, nseg;
  pairs_split(n, c0, c1, ctx->n_cu, dbg, &cpb, &nseg);
  if (nseg > (((int64_t)1 << 31) - 1) / pairs)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, std::string(who) + ": " + std::to_string(pairs) + " tile pairs x " + std::to_string(nseg) + " SNP segments exceed one grid");
  {
    const int64_t k0 = as_win(c0, M, W), k1 = as_win(c1 - 1, M, W) + 1, total = N * (k1 - k0);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)ctx->n_cu * 8));
    hipLaunchKernelGGL(k_ancestry_pairs_labels, dim3(grid), dim3(256), 0, s, d_labels, ld_labels, N, k0, k1, (int)A, d_bad);
    HIPCHK(ctx, hipGetLastError());
  }
  if (!d_DD && !d_DO && !d_OO) return GNX_OK;
  const int atomic = nseg > 1;
  if (atomic) {
    int32_t* tabs[3] = {d_DD, d_DO, d_OO};
    for (int32_t* tb : tabs)
      if (tb) HIPCHK(ctx, hipMemset2DAsync(tb, (size_t)ld * 4, 0, (size_t)n * 4, (size_t)n, s));
  }
  const int aligned = gnx_sum_rows_aligned(d_rows, row_kind, ld_rows);
  PairsLaunch L{(const uint8_t*)d_rows, d_labels, ld_rows, ld_labels, n, C, M, W, c0, c1, c0 / PR_KC * PR_KC, cpb, ld,
                ancestry, (int32_t)nseg, atomic, aligned, d_DD, d_DO, d_OO};
  const dim3 grid((unsigned)(pairs * nseg));
  if (row_kind == GNX_ROWS_PACKED2) hipLaunchKernelGGL(k_ancestry_pairs<GNX_ROWS_PACKED2>, grid, dim3(256), 0, s, L);
  else hipLaunchKernelGGL(k_ancestry_pairs<GNX_ROWS_INT8>, grid, dim3(256), 0, s, L);
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

// the tables of a host-pointer form: compact (n, n) slabs in ws_b32, NULL for a table the caller did not ask for
struct PairsHostBufs {
  int32_t *d_DD, *d_DO, *d_OO;
};

int pairs_host_bufs(gnx_ctx* ctx, int64_t n, const void* DD, const void* DO, const void* OO, PairsHostBufs* B) {
  const size_t tb = (((size_t)n * n * 4) + 255) & ~(size_t)255;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b32, 3 * tb + 64)) != GNX_OK) return rc;
  char* o = (char*)ctx->ws_b32.p;
  B->d_DD = DD ? (int32_t*)o : nullptr;
  B->d_DO = DO ? (int32_t*)(o + tb) : nullptr;
  B->d_OO = OO ? (int32_t*)(o + 2 * tb) : nullptr;
  return GNX_OK;
}

// the slabs and the count -> the host, one synchronisation
int pairs_copy_out(gnx_ctx* ctx, const PairsHostBufs& B, int64_t n, int32_t* DD, int32_t* DO, int32_t* OO, int64_t ld, const unsigned long long* d_bad,
                   unsigned long long* h_bad, hipStream_t s) {
  const size_t wb = (size_t)n * 4;
  if (DD) HIPCHK(ctx, hipMemcpy2DAsync(DD, (size_t)ld * 4, B.d_DD, wb, wb, (size_t)n, hipMemcpyDeviceToHost, s));
  if (DO) HIPCHK(ctx, hipMemcpy2DAsync(DO, (size_t)ld * 4, B.d_DO, wb, wb, (size_t)n, hipMemcpyDeviceToHost, s));
  if (OO) HIPCHK(ctx, hipMemcpy2DAsync(OO, (size_t)ld * 4, B.d_OO, wb, wb, (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(h_bad, d_bad, sizeof *h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_ancestry_pair_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                            int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1,
                                            int32_t* d_DD, int32_t* d_DO, int32_t* d_OO, int64_t ld, int64_t debug_snps_per_block, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const char* who = "ancestry_pair_counts";
  int rc = pairs_check(ctx, who, false, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, ancestry, c0, c1, ld, debug_snps_per_block);
  if (rc != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  unsigned long long* d_bad;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = pairs_run(ctx, who, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, ancestry, c0, c1, d_DD, d_DO, d_OO, ld,
                      debug_snps_per_block, d_bad, s)) != GNX_OK)
    return rc;
  return gnx_sum_read_verdict(ctx, who, d_bad, A, PR_TAIL, n_bad, s);
}

extern "C" int gnx_ancestry_pair_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                                        int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO,
                                        int32_t* OO, int64_t ld, int64_t debug_snps_per_block, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const char* who = "ancestry_pair_counts";
  int rc = pairs_check(ctx, who, false, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A, ancestry, c0, c1, ld, debug_snps_per_block);
  if (rc != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const int64_t n = N / 2;
  PairsHostBufs B;
  unsigned long long *d_bad, h_bad = 0;
  if ((rc = gnx_sum_stage_rows_labels(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = pairs_host_bufs(ctx, n, DD, DO, OO, &B)) != GNX_OK) return rc;
  if ((rc = pairs_run(ctx, who, ctx->ws_xu.p, row_kind, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, ancestry, c0, c1, B.d_DD, B.d_DO,
                      B.d_OO, n, debug_snps_per_block, d_bad, s)) != GNX_OK)
    return rc;
  if ((rc = pairs_copy_out(ctx, B, n, DD, DO, OO, ld, d_bad, &h_bad, s)) != GNX_OK) return rc;
  // (GNX_EINVAL here = labels out of range: the tables stand and were handed over)
  return gnx_sum_label_verdict(ctx, who, h_bad, A, PR_TAIL, n_bad);
}

// The file path's form.  A pair needs every row at once, so the WHOLE packed matrix is built in HBM, in device memory of this call's own
// (N rows of gnx_sum_gt2's pitch, freed on return), batch by batch with gnx_infer_gt2's staging (gnx_summary_host.h); the kernel then
// runs once.
extern "C" int gnx_ancestry_pair_counts_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels,
                                            int32_t ancestry, int64_t c0, int64_t c1, int32_t* DD, int32_t* DO, int32_t* OO, int64_t ld,
                                            int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  const char* who = "ancestry_pair_counts_gt2";
  int rc = gnx_sum_gt2_args(ctx, who, G, V, ldg, N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = pairs_check(ctx, who, true, nullptr, GNX_ROWS_PACKED2, (C + 3) / 4, labels, W, N, C, M, W, A, ancestry, c0, c1, ld, 0)) != GNX_OK) return rc;
  if ((rc = gnx_sum_check_src(ctx, who, src, C, V)) != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const int64_t n = N / 2;
  gnx_sum_gt2 st;
  gnx_sum_gt2_sizes(ctx, C, ldg, N, &st);
  {
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t need = (size_t)N * st.ldp + (size_t)V * st.ldg_d + 3 * (size_t)n * n * 4 + (size_t)N * W * 4 + (size_t)C * 4;
    if (need > total_b)
      return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_pair_counts_gt2: the packed rows of " + std::to_string(N) + " haplotypes plus the tables take " +
                                                 std::to_string(need) + " bytes, the device has " + std::to_string(total_b));
  }
  PairsHostBufs B;
  gnx_dev_tmp P;
  unsigned long long *d_bad, h_bad = 0;
  if ((rc = pairs_host_bufs(ctx, n, DD, DO, OO, &B)) != GNX_OK) return rc;
  if (P.alloc((size_t)N * st.ldp + 256) != hipSuccess)   // (before anything is enqueued)
    return gnx_fail(ctx, GNX_ENOMEM, "ancestry_pair_counts_gt2: no device memory for " + std::to_string((size_t)N * st.ldp) + " bytes of packed rows");
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, false, &st, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  HIPCHK(ctx, gnx_sum_gt2_all_rows(st, N, C, P.p, s));
  rc = pairs_run(ctx, who, P.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab, W, N, C, M, W, A, ancestry, c0, c1, B.d_DD, B.d_DO, B.d_OO, n, 0, d_bad, s);
  if (rc == GNX_OK) rc = pairs_copy_out(ctx, B, n, DD, DO, OO, ld, d_bad, &h_bad, s);
  else (void)hipStreamSynchronize(s);   // the rows are freed on return: nothing may still read them
  if (rc != GNX_OK) return rc;
  return gnx_sum_label_verdict(ctx, who, h_bad, A, PR_TAIL, n_bad);
}
