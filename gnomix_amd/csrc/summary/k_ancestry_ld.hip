// summary/k_ancestry_ld.hip — ancestry-specific linkage disequilibrium on the int8 matrix cores: for ONE ancestry a, the SNPs c of a range
// [c0, c1) and the offsets 0 <= k < band, four exact int32 sums over the haplotypes h, c' = c + k:
//   n11[c, k] = sum_h d[h, c] d[h, c']    n1o[c, k] = sum_h d[h, c] o[h, c']    no1[c, k] = sum_h o[h, c] d[h, c']    noo[c, k] = sum_h o[h, c] o[h, c']
// where, with win(c) = min(c / M, W - 1),
//   o[h, c] = 1 if labels[h, win(c)] == a AND the call is observed (code 0 or 1), else 0        d[h, c] = 1 if o[h, c] and the code is 1, else 0
// Every term is 0 or 1, so int32 is exact for every N < 2^31.  The host derives r and r^2 from them (gnomix_amd/ld.py).
// This is k_ancestry_pairs.hip turned on its side: that kernel contracts over SNPs and gives individual x individual tables, this one
// contracts over haplotypes and gives SNP x SNP tables, of which only a band beside the diagonal is kept.
//
// k_ancestry_ld<KIND>: a workgroup = 256 threads = 4 waves owns a tile I of LD_T = 64 SNPs and a tile J >= I of 64 SNPs (tiles start at
//   multiples of 64 from t0 = c0 rounded down to 64, so a group of 16 SNPs starts at a multiple of 16), and a SEGMENT of the haplotypes,
//   which it walks in chunks of LD_KC = 128.  J is one of the (band + 62) / 64 + 1 tiles I, I + 1, ... the band of I can reach (the last SNP
//   of I, 63, reaches 63 + band - 1); tiles that start at or beyond C hold nothing and are not launched (ld_geometry, ld_pair below).
//  * Fused, transposing staging.  The MFMA's K dimension is the haplotype, but a row of X is one haplotype.  An item is (4 consecutive
//    haplotypes, 16 SNPs): per haplotype one as_fields16 load and the mask of the SNPs whose window carries a (the pairs kernel's loop over
//    the windows that meet the 16 SNPs), d and o as ONE BIT per SNP; then per SNP the four haplotypes' bits are spread to the four bytes
//    of one dword, which is stored to image[snp][hap]: that store is the transposition.  Four images of 64 rows (d and o of I, d and o of
//    J); a diagonal pair stages its tile once and reads it for both operands.  No (N, C) intermediate exists in HBM.  Haplotypes >= N and
//    SNPs >= C are staged as zeros, which add nothing.  Nothing is read past a row's last byte (as_fields16) and a label is only compared
//    with a, never used as an index.
//  * Products.  Wave v owns rows 16 v .. 16 v + 15 of I and all four 16-column tiles of J: D_I D_J^T, D_I O_J^T, O_I D_J^T, O_I O_J^T, 16
//    accumulators of four int32, two v_mfma_i32_16x16x64_i8 steps per chunk.  Both operands are 16 consecutive bytes of a staged row (A:
//    row = lane & 15 of the wave's rows, B: row = lane & 15 of the column tile, k-block = lane >> 4), C/D: column = lane & 15, row =
//    4 (lane >> 4) + reg: k_ancestry_pairs' layout.  All four products are formed on the diagonal too: the band wants [c, c'] with
//    c' >= c of each, and O_I D_I^T is not D_I O_I^T.
//  * LDS pitch 160 bytes (LD_KC + 32), the READ side: k_ancestry_pairs' argument, unchanged, because the reads are the same.  A 16-byte read of
//    a wave is served in four groups of 16 lanes that hold every row r = lane & 15 once, the rows 0-3 and 12-15 with one k-block q and
//    the rows 4-11 with q + 1 (or the other way round).  In 16-byte slots, 16 of which make the 64 banks, row r and k-block q sit at
//    10 r + q: 10 r mod 16 takes each even value twice, for r and r + 8, exactly one of which lies in 4..11, so its + 1 makes the 16 slots
//    of a group distinct.
//  * The STORE side, which is new.  The staging stores are 4 bytes wide; such a store is served in two groups of 32 consecutive lanes, banked by
//    dword address mod 32.  Items are numbered so that the 32 lanes of a group hold the 32 haplotype quads of ONE group of 16 SNPs (thread
//    t: tile t / 128, SNP group (t / 32) % 4, quad t % 32): at each of its 16 stores a group writes the dwords 0 .. 31 of one staged row, 32
//    consecutive dwords = every bank once, whatever the pitch.  The other numbering (lanes along SNPs) would put lane l at l pitch / 4
//    mod 32 = 8 l mod 32 (pitch 160): 8-way.  (Both groupings are taken from public measurements of this chip; SQ_LDS_BANK_CONFLICT has not
//    been read on this kernel.)
//  * Stores.  Element (c, c') of a product goes to table[c - c0, c' - c] iff c0 <= c < c1, 0 <= c' - c < band and c' < C: the pair (I, J)
//    that holds (c, c') is unique, so every element has one owner.  Entries with c + k >= C have no owner; the host zeroes them first.
//  * The split over haplotype segments.  A short range or a small band gives few tile pairs (256 SNPs, band 64: 8 pairs for 256 CUs), so
//    the haplotypes are cut into segments of whole chunks and grid = pairs x segments.  The segments' sums are combined with int32 vector
//    atomic adds (global_atomic_add, no return value) into tables zeroed first; integer addition is associative, so the order cannot
//    change a sum.  Chosen over a workspace plus a reduce kernel for k_ancestry_pairs' reason: that costs segments x 4 tables written and
//    read again and one more launch.  One segment (many tile pairs) uses plain stores.
//  * Row reads (the known weak point, left as it is): a tile reads 16 bytes (int8) or 4 bytes (packed) per haplotype and group of 16 SNPs,
//    from rows ld_rows apart, and every J tile is staged again by each I that meets it.  DESIGN.md 4.22 says what the next step is.
// k_ancestry_ld_labels: the labels outside [0, A) in the windows the range and its band reach, counted for the verdict after the launch.
// No scratch, no runtime-indexed register array, plain vector stores or vector atomics only.  Index arithmetic is 64-bit throughout.
#include "gnx_summary_host.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int LD_T = 64;                               // SNPs per tile
constexpr int LD_KC = 128;                             // haplotypes per chunk: two steps of the MFMA's K = 64
constexpr int LD_P = LD_KC + 32;                       // LDS row pitch, bytes
constexpr int LD_IMG = LD_T * LD_P;                    // bytes of one staged image
constexpr int64_t LD_MIN_CHUNKS = 4;                   // chunks of a segment, at least (the built-in split)
constexpr uint32_t LD_EVEN = 0x55555555u;

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
  g.t0 = c0 / LD_T * LD_T;
  g.nI = (c1 - g.t0 + LD_T - 1) / LD_T;
  g.nJ = (band + 62) / LD_T + 1;
  g.nT = (C - g.t0 + LD_T - 1) / LD_T;                                  // >= nI
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

__device__ __forceinline__ void ld_put(int32_t* __restrict__ T, size_t at, int32_t v, int atomic) {
  if (atomic) atomicAdd(T + at, v);
  else T[at] = v;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_ancestry_ld(LdLaunch L) {
  __shared__ __attribute__((aligned(16))) uint8_t tz[4 * LD_IMG];  // d of tile I, o of tile I, d of tile J, o of tile J
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t pair = blockIdx.x / (uint32_t)L.nseg, seg = blockIdx.x - pair * (uint32_t)L.nseg;
  int64_t bi, dj;
  ld_pair(L, (int64_t)pair, &bi, &dj);
  const bool diag = dj == 0;
  const int64_t iI = L.t0 + bi * LD_T, iJ = iI + dj * LD_T;                  // the tiles' first SNPs; iJ < C by the grid
  const int64_t h0 = (int64_t)seg * L.cpb * LD_KC;                           // < N by the grid
  const int64_t h1 = (h0 + L.cpb * LD_KC < L.N) ? h0 + L.cpb * LD_KC : L.N;

  v4i dd[4], dx[4], xd[4], oo[4];   // D_I D_J^T, D_I O_J^T, O_I D_J^T, O_I O_J^T
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) dd[jt] = dx[jt] = xd[jt] = oo[jt] = v4i{0, 0, 0, 0};
  const uint8_t* ap = tz + (wv * 16 + (lane & 15)) * LD_P + (lane >> 4) * 16;
  const uint8_t* bp = tz + (diag ? 0 : 2 * LD_IMG) + (lane & 15) * LD_P + (lane >> 4) * 16;

  // this thread's item: tile, group of 16 SNPs, quad of haplotypes
  const int tile = t >> 7, g = (t >> 5) & 3, q = t & 31;
  const int64_t cg = (tile ? iJ : iI) + 16 * g;                              // a multiple of 16
  const int64_t hi = cg + 16 < L.C ? cg + 16 : L.C;
  const bool stages = (tile == 0 || !diag) && cg < L.C;                      // (a group at or beyond C stays zero: zeroed once, below)
  uint8_t* const dst = tz + (2 * tile) * LD_IMG + (16 * g) * LD_P + 4 * q;
  if (!stages && (tile == 0 || !diag)) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      *reinterpret_cast<uint32_t*>(dst + j * LD_P) = 0u;
      *reinterpret_cast<uint32_t*>(dst + LD_IMG + j * LD_P) = 0u;
    }
  }

  for (int64_t k0 = h0; k0 < h1; k0 += LD_KC) {
    if (stages) {
      uint32_t d01 = 0, d23 = 0, o01 = 0, o23 = 0;      // bits 2 j, 2 j + 1 = SNP j of the quad's haplotypes 0, 1 (2, 3)
#pragma unroll
      for (int hq = 0; hq < 4; ++hq) {
        const int64_t h = k0 + 4 * q + hq;
        uint32_t db = 0, ob = 0;
        if (h < h1) {
          const uint32_t f = as_fields16<KIND>(L.rows + h * L.ld, cg, L.C, L.aligned);
          const uint32_t obs = ~(f >> 1) & LD_EVEN, alt = f & obs;
          const int32_t* lh = L.lab + h * L.ldl;
          uint32_t m = 0;
          int64_t c = cg, k = cg / L.M;
          if (k > L.W - 1) k = L.W - 1;
          while (c < hi) {          // the SNPs [c, se) lie in window k
            const int64_t wend = (k == L.W - 1) ? L.C : (k + 1) * L.M;
            const int64_t se = hi < wend ? hi : wend;
            if (lh[k] == L.a) m |= as_range16((int)(c - cg), (int)(se - cg));
            c = se;
            ++k;
          }
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
        *reinterpret_cast<uint32_t*>(dst + j * LD_P) = wd;
        *reinterpret_cast<uint32_t*>(dst + LD_IMG + j * LD_P) = wo;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < LD_KC / 64; ++ks) {
      const v4i ad = *reinterpret_cast<const v4i*>(ap + 64 * ks);
      const v4i ao = *reinterpret_cast<const v4i*>(ap + LD_IMG + 64 * ks);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const v4i bd = *reinterpret_cast<const v4i*>(bp + jt * 16 * LD_P + 64 * ks);
        const v4i bo = *reinterpret_cast<const v4i*>(bp + LD_IMG + jt * 16 * LD_P + 64 * ks);
        dd[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bd, dd[jt], 0, 0, 0);
        dx[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bo, dx[jt], 0, 0, 0);
        xd[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bd, xd[jt], 0, 0, 0);
        oo[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bo, oo[jt], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const size_t ldt = (size_t)L.ldt;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t c = iI + wv * 16 + 4 * (lane >> 4) + r;
      const int64_t c2 = iJ + jt * 16 + (lane & 15);
      const int64_t k = c2 - c;
      if (c < L.c0 || c >= L.c1 || k < 0 || k >= L.band || c2 >= L.C) continue;
      const size_t at = (size_t)(c - L.c0) * ldt + (size_t)k;
      if (L.n11) ld_put(L.n11, at, dd[jt][r], L.atomic);
      if (L.n1o) ld_put(L.n1o, at, dx[jt][r], L.atomic);
      if (L.no1) ld_put(L.no1, at, xd[jt][r], L.atomic);
      if (L.noo) ld_put(L.noo, at, oo[jt][r], L.atomic);
    }
}

// labels outside [0, A) among the rows' windows [k0, k1)
__global__ __launch_bounds__(256) void k_ancestry_ld_labels(const int32_t* __restrict__ lab, int64_t ldl, int64_t N, int64_t k0, int64_t k1, int A,
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

const char* const LD_TAIL = "such a haplotype counts for no ancestry at that window";

// every refusal that needs no device memory; GNX_OK or the code.  built: the rows are built by this call (the file path's form)
int ld_check(gnx_ctx* ctx, const char* who, bool built, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N,
             int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int64_t ld, int64_t dbg) {
  const std::string w(who);
  const int rc = gnx_sum_geometry_check(ctx, who, built ? GNX_SUM_ROWS_BUILT : 0u, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A);
  if (rc != GNX_OK) return rc;
  if (ancestry < 0 || ancestry >= A) return gnx_fail(ctx, GNX_EINVAL, w + ": ancestry outside [0, A)");
  if (c0 < 0 || c1 <= c0 || c1 > C) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= c0 < c1 <= C");
  if (band < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": band must be >= 1");
  if (ld < band) return gnx_fail(ctx, GNX_EINVAL, w + ": the tables' row stride is smaller than band");
  if (N >= ((int64_t)1 << 31)) return gnx_fail(ctx, GNX_EINVAL, w + ": N must be below 2^31");
  if (dbg < 0) return gnx_fail(ctx, GNX_EINVAL, w + ": the debug argument must be >= 0 (0 = the built-in choice)");
  if (A > GNX_ALLELE_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, at most " + std::to_string(GNX_ALLELE_MAX_A));
  if (band > GNX_LD_MAX_BAND) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": band = " + std::to_string(band) + ", at most " + std::to_string(GNX_LD_MAX_BAND));
  return GNX_OK;
}

// the split of the N haplotypes: chunks per segment and the number of segments, a function of (N, pairs, n_cu, dbg) alone
void ld_split(int64_t N, int64_t pairs, int n_cu, int64_t dbg, int64_t* cpb, int64_t* nseg) {
  const int64_t chunks = (N + LD_KC - 1) / LD_KC;
  int64_t per = chunks;
  if (dbg > 0) {
    per = (dbg + LD_KC - 1) / LD_KC;
  } else {
    const int64_t want = (int64_t)n_cu * 4;            // about four workgroups per CU
    if (pairs < want) {
      const int64_t ns = (want + pairs - 1) / pairs;   // segments that would fill the chip
      per = std::max(LD_MIN_CHUNKS, (chunks + ns - 1) / ns);
    }
  }
  per = std::min(per, chunks);
  *cpb = per;
  *nseg = (chunks + per - 1) / per;
}

// the tables of N > 0 rows (device pointers, any table may be NULL), and the labels out of range ADDED to *d_bad.  Arguments checked.
int ld_run(gnx_ctx* ctx, const char* who, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N,
           int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* d_n11, int32_t* d_n1o,
           int32_t* d_no1, int32_t* d_noo, int64_t ld, int64_t dbg, unsigned long long* d_bad, hipStream_t s) {
  const LdGeometry g = ld_geometry(C, c0, c1, band);
  int64_t cpb, nseg;
  ld_split(N, g.pairs, ctx->n_cu, dbg, &cpb, &nseg);
  if (nseg > (((int64_t)1 << 31) - 1) / g.pairs)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, std::string(who) + ": " + std::to_string(g.pairs) + " tile pairs x " + std::to_string(nseg) + " haplotype segments exceed one grid");
  {
    const int64_t last = std::min(c1 - 1 + band - 1, C - 1);     // the last SNP the band reaches
    const int64_t k0 = as_win(c0, M, W), k1 = as_win(last, M, W) + 1, total = N * (k1 - k0);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)ctx->n_cu * 8));
    hipLaunchKernelGGL(k_ancestry_ld_labels, dim3(grid), dim3(256), 0, s, d_labels, ld_labels, N, k0, k1, (int)A, d_bad);
    HIPCHK(ctx, hipGetLastError());
  }
  if (!d_n11 && !d_n1o && !d_no1 && !d_noo) return GNX_OK;
  const int atomic = nseg > 1;
  // zeroed first: everything where the segments add; else the rows whose band reaches beyond C (those entries have no owner)
  const int64_t z0 = atomic ? 0 : std::max(c0, C - band + 1) - c0;
  if (z0 < c1 - c0) {
    int32_t* tabs[4] = {d_n11, d_n1o, d_no1, d_noo};
    for (int32_t* tb : tabs)
      if (tb) HIPCHK(ctx, hipMemset2DAsync(tb + (size_t)z0 * (size_t)ld, (size_t)ld * 4, 0, (size_t)band * 4, (size_t)(c1 - c0 - z0), s));
  }
  const int aligned = gnx_sum_rows_aligned(d_rows, row_kind, ld_rows);
  LdLaunch L{(const uint8_t*)d_rows, d_labels, ld_rows, ld_labels, N, C, M, W, c0, c1, g.t0, band, cpb, ld, g.nJ, g.nT, g.full,
             ancestry, (int32_t)nseg, atomic, aligned, d_n11, d_n1o, d_no1, d_noo};
  const dim3 grid((unsigned)(g.pairs * nseg));
  if (row_kind == GNX_ROWS_PACKED2) hipLaunchKernelGGL(k_ancestry_ld<GNX_ROWS_PACKED2>, grid, dim3(256), 0, s, L);
  else hipLaunchKernelGGL(k_ancestry_ld<GNX_ROWS_INT8>, grid, dim3(256), 0, s, L);
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

// the tables of a host-pointer form: compact (c1 - c0, band) slabs in ws_b32, NULL for a table the caller did not ask for
struct LdHostBufs {
  int32_t* d[4];
};

int ld_host_bufs(gnx_ctx* ctx, int64_t nc, int64_t band, int32_t* const host[4], LdHostBufs* B) {
  const size_t tb = (((size_t)nc * (size_t)band * 4) + 255) & ~(size_t)255;
  const int rc = gnx_ws_reserve(ctx, ctx->ws_b32, 4 * tb + 64);
  if (rc != GNX_OK) return rc;
  char* o = (char*)ctx->ws_b32.p;
  for (int q = 0; q < 4; ++q) B->d[q] = host[q] ? (int32_t*)(o + q * tb) : nullptr;
  return GNX_OK;
}

// the slabs and the count -> the host, one synchronisation
int ld_copy_out(gnx_ctx* ctx, const LdHostBufs& B, int64_t nc, int64_t band, int32_t* const host[4], int64_t ld, const unsigned long long* d_bad,
                unsigned long long* h_bad, hipStream_t s) {
  const size_t wb = (size_t)band * 4;
  for (int q = 0; q < 4; ++q)
    if (host[q]) HIPCHK(ctx, hipMemcpy2DAsync(host[q], (size_t)ld * 4, B.d[q], wb, wb, (size_t)nc, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(h_bad, d_bad, sizeof *h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_ancestry_ld_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                          int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band,
                                          int32_t* d_n11, int32_t* d_n1o, int32_t* d_no1, int32_t* d_noo, int64_t ld, int64_t debug_haps_per_block,
                                          int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const char* who = "ancestry_ld_counts";
  int rc = ld_check(ctx, who, false, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, ancestry, c0, c1, band, ld, debug_haps_per_block);
  if (rc != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  unsigned long long* d_bad;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = ld_run(ctx, who, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, ancestry, c0, c1, band, d_n11, d_n1o, d_no1, d_noo, ld,
                   debug_haps_per_block, d_bad, s)) != GNX_OK)
    return rc;
  return gnx_sum_read_verdict(ctx, who, d_bad, A, LD_TAIL, n_bad, s);
}

extern "C" int gnx_ancestry_ld_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                                      int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11,
                                      int32_t* n1o, int32_t* no1, int32_t* noo, int64_t ld, int64_t debug_haps_per_block, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  const char* who = "ancestry_ld_counts";
  int rc = ld_check(ctx, who, false, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A, ancestry, c0, c1, band, ld, debug_haps_per_block);
  if (rc != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  int32_t* const host[4] = {n11, n1o, no1, noo};
  LdHostBufs B;
  unsigned long long *d_bad, h_bad = 0;
  if ((rc = gnx_sum_stage_rows_labels(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = ld_host_bufs(ctx, c1 - c0, band, host, &B)) != GNX_OK) return rc;
  if ((rc = ld_run(ctx, who, ctx->ws_xu.p, row_kind, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, ancestry, c0, c1, band, B.d[0],
                   B.d[1], B.d[2], B.d[3], band, debug_haps_per_block, d_bad, s)) != GNX_OK)
    return rc;
  if ((rc = ld_copy_out(ctx, B, c1 - c0, band, host, ld, d_bad, &h_bad, s)) != GNX_OK) return rc;
  // (GNX_EINVAL here = labels out of range: the tables stand and were handed over)
  return gnx_sum_label_verdict(ctx, who, h_bad, A, LD_TAIL, n_bad);
}

// The file path's form.  The sums run over every row, so the WHOLE packed matrix is built in HBM, in device memory of this call's own
// (N rows of gnx_sum_gt2's pitch, freed on return), batch by batch with gnx_infer_gt2's staging (gnx_summary_host.h); the kernel then
// runs once.
extern "C" int gnx_ancestry_ld_counts_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels,
                                          int32_t ancestry, int64_t c0, int64_t c1, int64_t band, int32_t* n11, int32_t* n1o, int32_t* no1, int32_t* noo,
                                          int64_t ld, int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  const char* who = "ancestry_ld_counts_gt2";
  int rc = gnx_sum_gt2_args(ctx, who, G, V, ldg, N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = ld_check(ctx, who, true, nullptr, GNX_ROWS_PACKED2, (C + 3) / 4, labels, W, N, C, M, W, A, ancestry, c0, c1, band, ld, 0)) != GNX_OK) return rc;
  if ((rc = gnx_sum_check_src(ctx, who, src, C, V)) != GNX_OK) return rc;
  if (n_bad) *n_bad = 0;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const int64_t nc = c1 - c0;
  gnx_sum_gt2 st;
  gnx_sum_gt2_sizes(ctx, C, ldg, N, &st);
  {
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t need = (size_t)N * st.ldp + (size_t)V * st.ldg_d + 4 * (size_t)nc * (size_t)band * 4 + (size_t)N * W * 4 + (size_t)C * 4;
    if (need > total_b)
      return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_ld_counts_gt2: the packed rows of " + std::to_string(N) + " haplotypes plus the tables take " +
                                                 std::to_string(need) + " bytes, the device has " + std::to_string(total_b));
  }
  int32_t* const host[4] = {n11, n1o, no1, noo};
  LdHostBufs B;
  gnx_dev_tmp P;
  unsigned long long *d_bad, h_bad = 0;
  if ((rc = ld_host_bufs(ctx, nc, band, host, &B)) != GNX_OK) return rc;
  if (P.alloc((size_t)N * st.ldp + 256) != hipSuccess)   // (before anything is enqueued)
    return gnx_fail(ctx, GNX_ENOMEM, "ancestry_ld_counts_gt2: no device memory for " + std::to_string((size_t)N * st.ldp) + " bytes of packed rows");
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, false, &st, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  HIPCHK(ctx, gnx_sum_gt2_all_rows(st, N, C, P.p, s));
  rc = ld_run(ctx, who, P.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab, W, N, C, M, W, A, ancestry, c0, c1, band, B.d[0], B.d[1], B.d[2], B.d[3], band, 0, d_bad, s);
  if (rc == GNX_OK) rc = ld_copy_out(ctx, B, nc, band, host, ld, d_bad, &h_bad, s);
  else (void)hipStreamSynchronize(s);   // the rows are freed on return: nothing may still read them
  if (rc != GNX_OK) return rc;
  return gnx_sum_label_verdict(ctx, who, h_bad, A, LD_TAIL, n_bad);
}
