// summary/k_allele_counts.hip — the join of a local-ancestry call with the genotypes it was made from: ancestry-specific allele counts
// per SNP and the per-individual, per-ancestry dosage / haplotype-count matrices, for rows and labels that are in HBM.
//
// X (N, C) in the model's coding, as int8 rows (0 = REF, 1 = ALT, any other byte = missing) or as 2-bit rows (gnx_pack_x layout: SNP j =
// bits 2 (j % 4).. of byte j / 4; codes 2 and 3 = missing).  labels (N, W) int32; the window of SNP c is win(c) = min(c / M, W - 1).
//   n_obs[a, c]  = #{h : labels[h, win(c)] == a, X[h, c] in {0, 1}}      n_alt[a, c] = #{h : ... , X[h, c] == 1}
//   n_miss[a, c] = #{h : labels[h, win(c)] == a, X[h, c] not in {0, 1}}   (three (A, C) int32 tables)
//   hapcount[i, c] = how many of the haplotypes 2 i, 2 i + 1 carry label a at win(c); dosage[i, c] = how many of those have code 1
//
// k_ancestry_allele_counts<KIND>: a column reduction over N.  A workgroup is ONE wave; it owns a tile of AC_TILE = 1024 columns and a chunk
// of rows.  Lane l owns the 16 adjacent columns 16 l.. of the tile: one 32-bit load of a packed row (one 16-byte load of an int8 row,
// re-coded to the same 16 2-bit fields).  Counters are BYTES in LDS, [A][3 tables: all, alt, miss][64 lanes][16 columns]: a lane's 16
// counters of one (ancestry, table) are one 16-byte slot at 16 l + constant, read and written whole (conflict-free), and a lane only ever
// touches its own slots, so the read-modify-write needs no atomics.  The 16 fields become 0 / 1 bytes with one multiply per four.
// The rows of a chunk go in batches of at most `flush_every` <= 255 rows (a byte cannot overflow) and of at most AC_LAB_BYTES / (windows
// the tile spans) rows: per batch the wave stages the labels of those rows and windows in LDS as bytes (a label outside [0, A) becomes
// 0xff: labels are only compared, never used as an index), counts, and then adds the batch's counters to the global int32 tables, lane
// = column, 256 contiguous bytes per atomic instruction, zeros skipped (n_obs = all - miss).  Integer adds commute: the tables do not
// depend on the geometry.  A tile spans at most 1024 windows (M = 1), so a batch always holds at least four rows: small M only means
// more, smaller batches.  A lane whose 16 columns lie in more than one window (M < 16, or a border inside its group, also inside one
// packed byte) takes the per-column route: one byte counter at a time.  Columns >= C are masked out of every table.
//
// k_ancestry_dosage<KIND>: elementwise, one thread per (individual, group of 16 columns): both rows' 16 fields, both labels (per column
// where the group spans a window border), two 16-byte stores.
//
// Neither kernel has a per-thread array that is indexed at run time; no scratch.
#include "gnx_summary_host.h"

namespace {

constexpr int AC_THREADS = 64;
constexpr int AC_COLS = 16;                        // columns a lane owns: one packed 32-bit word
constexpr int AC_TILE = AC_THREADS * AC_COLS;      // 1024 columns per workgroup
constexpr int AC_LAB_BYTES = 4096;                 // staged labels of one batch (>= 4 rows: a tile spans <= 1024 windows)
constexpr int AC_MAX_FLUSH = 255;                  // rows a byte counter takes
constexpr int AC_MAX_A = GNX_ALLELE_MAX_A;
constexpr uint32_t EVEN = 0x55555555u, ONES = 0x01010101u;

// fields 4 q .. 4 q + 3 of x (one bit each, at the even positions) -> the four bytes of a word, 0 or 1 each: the bits 0, 2, 4, 6 of the
// byte move up by 0, 6, 12, 18 (two partial products meet only at bits 6, 12 and 18, and their carry ends in an empty odd bit)
__device__ __forceinline__ uint32_t spread(uint32_t x, int q) { return (((x >> (8 * q)) & 0x55u) * 0x00041041u) & ONES; }

// 0x01 in the bytes of the valid ones of the columns 4 k .. 4 k + 3 of a group with nvalid valid columns
__device__ __forceinline__ uint32_t valid_bytes(int nvalid, int k) {
  const int n = nvalid - 4 * k;
  return n >= 4 ? ONES : n <= 0 ? 0u : (ONES & ((1u << (8 * n)) - 1u));
}

template <int KIND>
__global__ __launch_bounds__(AC_THREADS) void k_ancestry_allele_counts(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lab,
                                                                       int64_t ldl, int64_t N, int64_t C, int64_t M, int64_t W, int A,
                                                                       int64_t n_ctiles, int64_t rows_per_chunk, int flush_every, int aligned,
                                                                       int32_t* __restrict__ n_obs, int32_t* __restrict__ n_alt,
                                                                       int32_t* __restrict__ n_miss, unsigned long long* __restrict__ bad) {
  extern __shared__ uint4 ac_lds[];              // counters: [A][3][64 lanes] slots of 16 bytes; then AC_LAB_BYTES label bytes
  uint4* cnt = ac_lds;
  uint8_t* cnt8 = reinterpret_cast<uint8_t*>(ac_lds);
  uint8_t* slab = cnt8 + (size_t)A * 3 * AC_TILE;
  const int lane = threadIdx.x;
  const int64_t ct = blockIdx.x % n_ctiles, ch = blockIdx.x / n_ctiles;
  const int64_t t0 = ct * AC_TILE, t1 = (t0 + AC_TILE < C) ? t0 + AC_TILE : C;   // the tile's columns [t0, t1), t1 > t0
  const int64_t r_begin = ch * rows_per_chunk, r_end = (r_begin + rows_per_chunk < N) ? r_begin + rows_per_chunk : N;
  const int64_t w0 = (t0 / M < W - 1) ? t0 / M : W - 1, w1 = ((t1 - 1) / M < W - 1) ? (t1 - 1) / M : W - 1;
  const int nw = (int)(w1 - w0 + 1);             // windows the tile spans, <= AC_TILE
  const int by_lab = AC_LAB_BYTES / nw;
  const int batch = flush_every < by_lab ? flush_every : by_lab;
  const int ncols = (int)(t1 - t0);
  // this lane's group of columns
  const int64_t c0 = t0 + AC_COLS * lane;
  const int nvalid = (int)((C - c0 >= AC_COLS) ? AC_COLS : (C - c0 > 0 ? C - c0 : 0));
  const int64_t wa = (c0 / M < W - 1) ? c0 / M : W - 1;                 // window of the group's first column
  const int64_t cl = c0 + (nvalid > 0 ? nvalid - 1 : 0);
  const bool one_window = ((cl / M < W - 1) ? cl / M : W - 1) == wa;
  const int lw = (int)(wa - w0);                 // (only used where nvalid > 0: then 0 <= lw < nw)
  const uint32_t vm0 = valid_bytes(nvalid, 0), vm1 = valid_bytes(nvalid, 1), vm2 = valid_bytes(nvalid, 2), vm3 = valid_bytes(nvalid, 3);
  unsigned int my_bad = 0;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += batch) {
    const int nb = (int)((r_end - r0 < batch) ? r_end - r0 : batch);
    for (int i = lane; i < A * 3 * AC_THREADS; i += AC_THREADS) cnt[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = lane; i < nb * nw; i += AC_THREADS) {
      const int r = i / nw, k = i - r * nw;
      const int32_t v = lab[(r0 + r) * ldl + w0 + k];
      const bool ok = v >= 0 && v < A;
      slab[i] = ok ? (uint8_t)v : (uint8_t)0xff;
      // a label is reported once: by the tile that holds its window's first column
      if (!ok) {
        const int64_t f = (w0 + k) * M;
        if (f >= t0 && f < t1) ++my_bad;
      }
    }
    __syncthreads();
    if (nvalid > 0) {
      for (int rb = 0; rb < nb; rb += 4) {
        uint32_t f0 = 0, f1 = 0, f2 = 0, f3 = 0;   // four rows' loads in flight before the first is used
        f0 = as_fields16<KIND>(rows + (r0 + rb) * ld, c0, C, aligned);
        if (rb + 1 < nb) f1 = as_fields16<KIND>(rows + (r0 + rb + 1) * ld, c0, C, aligned);
        if (rb + 2 < nb) f2 = as_fields16<KIND>(rows + (r0 + rb + 2) * ld, c0, C, aligned);
        if (rb + 3 < nb) f3 = as_fields16<KIND>(rows + (r0 + rb + 3) * ld, c0, C, aligned);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (rb + u >= nb) break;
          const uint32_t f = u == 0 ? f0 : u == 1 ? f1 : u == 2 ? f2 : f3;
          const uint32_t hi = (f >> 1) & EVEN, alt = f & EVEN & ~hi;  // hi: codes 2 and 3 = missing
          const uint8_t* lrow = slab + (rb + u) * nw;
          if (one_window) {
            const int a = lrow[lw];
            if (a != 0xff) {
              uint4* p = cnt + (a * 3) * AC_THREADS + lane;
              uint4 v = p[0];
              v.x += vm0; v.y += vm1; v.z += vm2; v.w += vm3;
              p[0] = v;
              v = p[AC_THREADS];
              v.x += spread(alt, 0) & vm0; v.y += spread(alt, 1) & vm1; v.z += spread(alt, 2) & vm2; v.w += spread(alt, 3) & vm3;
              p[AC_THREADS] = v;
              v = p[2 * AC_THREADS];
              v.x += spread(hi, 0) & vm0; v.y += spread(hi, 1) & vm1; v.z += spread(hi, 2) & vm2; v.w += spread(hi, 3) & vm3;
              p[2 * AC_THREADS] = v;
            }
          } else {
            int wn = lw;                              // window of column c0 + j, relative to w0
            int64_t next = (wa + 1) * M;              // first column of the next window
            for (int j = 0; j < nvalid; ++j) {
              while (c0 + j >= next && w0 + wn < W - 1) { ++wn; next += M; }
              const int a = lrow[wn];
              if (a != 0xff) {
                uint8_t* q = cnt8 + ((size_t)(a * 3) * AC_THREADS + lane) * 16 + j;
                q[0] += 1;
                if ((alt >> (2 * j)) & 1u) q[AC_TILE] += 1;
                if ((hi >> (2 * j)) & 1u) q[2 * AC_TILE] += 1;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    // the batch's counters -> the global tables: lane = column, 64 adjacent int32 per instruction
    for (int a = 0; a < A; ++a) {
      const uint8_t* q = cnt8 + (size_t)(a * 3) * AC_TILE;
      const int64_t g = (int64_t)a * C + t0;
      for (int i = lane; i < ncols; i += AC_THREADS) {
        const int all = q[i], na = q[AC_TILE + i], nm = q[2 * AC_TILE + i];
        if (n_obs && all != nm) atomicAdd(&n_obs[g + i], all - nm);
        if (n_alt && na) atomicAdd(&n_alt[g + i], na);
        if (n_miss && nm) atomicAdd(&n_miss[g + i], nm);
      }
    }
    __syncthreads();
  }
  if (my_bad) atomicAdd(bad, (unsigned long long)my_bad);
}

// the fields (even bits) of the columns c0 .. c0 + n - 1 whose window's label in row `lab` equals anc; labels outside [0, A) are counted
// once each, by the group that holds their window's first column
__device__ __forceinline__ uint32_t select_fields(const int32_t* __restrict__ lab, int64_t c0, int n, int64_t M, int64_t W, int A, int anc,
                                                  unsigned int* n_bad) {
  const int64_t wa = (c0 / M < W - 1) ? c0 / M : W - 1;
  const int64_t cl = c0 + n - 1;
  if (((cl / M < W - 1) ? cl / M : W - 1) == wa) {
    const int32_t v = lab[wa];
    if ((v < 0 || v >= A) && wa * M == c0) ++*n_bad;
    return v == anc ? EVEN : 0u;
  }
  uint32_t sel = 0;
  int64_t wn = wa, next = (wa + 1) * M;
  int32_t v = lab[wn];
  if ((v < 0 || v >= A) && wa * M == c0) ++*n_bad;
  for (int j = 0; j < n; ++j) {
    if (c0 + j >= next && wn < W - 1) {   // (M >= 1: a column enters at most one new window)
      ++wn;
      next += M;
      v = lab[wn];
      if (v < 0 || v >= A) ++*n_bad;
    }
    if (v == anc) sel |= 1u << (2 * j);
  }
  return sel;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_ancestry_dosage(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lab, int64_t ldl,
                                                         int64_t n_ind, int64_t C, int64_t M, int64_t W, int A, int anc, int64_t G, int aligned_in,
                                                         uint8_t* __restrict__ dosage, int64_t ld_d, uint8_t* __restrict__ hapcount,
                                                         int64_t ld_h, int aligned_out, unsigned long long* __restrict__ bad) {
  const int64_t total = n_ind * G;
  unsigned int my_bad = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / G, g = e - i * G;
    const int64_t c0 = g * AC_COLS;
    const int n = (int)((C - c0 < AC_COLS) ? C - c0 : AC_COLS);
    const uint32_t fa = as_fields16<KIND>(rows + (2 * i) * ld, c0, C, aligned_in);
    const uint32_t fb = as_fields16<KIND>(rows + (2 * i + 1) * ld, c0, C, aligned_in);
    const uint32_t sa = select_fields(lab + (2 * i) * ldl, c0, n, M, W, A, anc, &my_bad);
    const uint32_t sb = select_fields(lab + (2 * i + 1) * ldl, c0, n, M, W, A, anc, &my_bad);
    const uint32_t alt_a = fa & EVEN & ~((fa >> 1) & EVEN) & sa, alt_b = fb & EVEN & ~((fb >> 1) & EVEN) & sb;
    const uint4 d = make_uint4(spread(alt_a, 0) + spread(alt_b, 0), spread(alt_a, 1) + spread(alt_b, 1), spread(alt_a, 2) + spread(alt_b, 2),
                               spread(alt_a, 3) + spread(alt_b, 3));
    const uint4 h = make_uint4(spread(sa, 0) + spread(sb, 0), spread(sa, 1) + spread(sb, 1), spread(sa, 2) + spread(sb, 2),
                               spread(sa, 3) + spread(sb, 3));
    uint8_t* pd = dosage ? dosage + i * ld_d + c0 : nullptr;
    uint8_t* ph = hapcount ? hapcount + i * ld_h + c0 : nullptr;
    if (aligned_out && n == AC_COLS) {
      if (pd) *reinterpret_cast<uint4*>(pd) = d;
      if (ph) *reinterpret_cast<uint4*>(ph) = h;
    } else {
      for (int j = 0; j < n; ++j) {
        const uint32_t dw = j < 4 ? d.x : j < 8 ? d.y : j < 12 ? d.z : d.w;
        const uint32_t hw = j < 4 ? h.x : j < 8 ? h.y : j < 12 ? h.z : h.w;
        if (pd) pd[j] = (uint8_t)(dw >> (8 * (j & 3)));
        if (ph) ph[j] = (uint8_t)(hw >> (8 * (j & 3)));
      }
    }
  }
  if (my_bad) atomicAdd(bad, (unsigned long long)my_bad);
}

const char* const AC_TAIL = "such a label counts for no ancestry";

// the checks the counts and the dosage share; GNX_OK or the refusal
int geometry_check(gnx_ctx* ctx, const char* who, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N,
                   int64_t C, int64_t M, int64_t W, int32_t A) {
  const std::string w(who);
  const int rc = gnx_sum_geometry_check(ctx, who, 0, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A);
  if (rc != GNX_OK) return rc;
  if (N >= ((int64_t)1 << 31)) return gnx_fail(ctx, GNX_EINVAL, w + ": N must be below 2^31");
  if (A > AC_MAX_A)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, a staged label is compared with at most " +
                                               std::to_string(AC_MAX_A) + " classes");
  return GNX_OK;
}

int counts_check(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N, int64_t C, int64_t M,
                 int64_t W, int32_t A, int64_t rpc, int64_t fe) {
  int rc = geometry_check(ctx, "ancestry_allele_counts", rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A);
  if (rc != GNX_OK) return rc;
  if (rpc < 0 || fe < 0) return gnx_fail(ctx, GNX_EINVAL, "ancestry_allele_counts: the debug arguments must be >= 0 (0 = the built-in choice)");
  if (A > ((int64_t)1 << 31) / C) return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_allele_counts: A * C must stay below 2^31");
  return GNX_OK;
}

int zero_tables(gnx_ctx* ctx, int32_t A, int64_t C, int32_t* d_obs, int32_t* d_alt, int32_t* d_miss, hipStream_t s) {
  const size_t b = (size_t)A * (size_t)C * sizeof(int32_t);
  if (d_obs) HIPCHK(ctx, hipMemsetAsync(d_obs, 0, b, s));
  if (d_alt) HIPCHK(ctx, hipMemsetAsync(d_alt, 0, b, s));
  if (d_miss) HIPCHK(ctx, hipMemsetAsync(d_miss, 0, b, s));
  return GNX_OK;
}

}  // namespace

// adds the counts of N rows to the tables (which the caller has zeroed) and the number of out-of-range labels to *d_bad; arguments checked
// by the caller
static hipError_t gnx_launch_allele_counts(const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t N,
                                    int64_t C, int64_t M, int64_t W, int32_t A, int32_t* d_obs, int32_t* d_alt, int32_t* d_miss,
                                    int64_t rows_per_chunk, int64_t flush_every, unsigned long long* d_bad, int n_cu, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  const int64_t n_ctiles = (C + AC_TILE - 1) / AC_TILE;
  int64_t rpc = rows_per_chunk;
  if (rpc <= 0) {  // about eight waves per CU, and no chunk shorter than one full batch of rows
    const int64_t want = std::max<int64_t>(1, ((int64_t)n_cu * 8 + n_ctiles - 1) / n_ctiles);
    const int64_t n_chunks = std::max<int64_t>(1, std::min<int64_t>(want, N / AC_MAX_FLUSH));
    rpc = (N + n_chunks - 1) / n_chunks;
  }
  const int64_t n_chunks = (N + rpc - 1) / rpc;
  if (n_chunks > ((int64_t)1 << 31) / n_ctiles - 1) return hipErrorInvalidConfiguration;
  const int fe = (int)(flush_every > 0 ? std::min<int64_t>(flush_every, AC_MAX_FLUSH) : AC_MAX_FLUSH);
  const size_t lds = (size_t)A * 3 * AC_TILE + AC_LAB_BYTES;
  const int aligned = gnx_sum_rows_aligned(d_rows, row_kind, ld_rows);
  const dim3 grid((unsigned)(n_ctiles * n_chunks));
  const uint8_t* rows = (const uint8_t*)d_rows;
  if (row_kind == GNX_ROWS_PACKED2) {
    GNX_LDS_OPTIN(lds, k_ancestry_allele_counts<GNX_ROWS_PACKED2>);
    hipLaunchKernelGGL(k_ancestry_allele_counts<GNX_ROWS_PACKED2>, grid, dim3(AC_THREADS), lds, s, rows, ld_rows, d_labels, ld_labels, N, C, M, W,
                       (int)A, n_ctiles, rpc, fe, aligned, d_obs, d_alt, d_miss, d_bad);
  } else {
    GNX_LDS_OPTIN(lds, k_ancestry_allele_counts<GNX_ROWS_INT8>);
    hipLaunchKernelGGL(k_ancestry_allele_counts<GNX_ROWS_INT8>, grid, dim3(AC_THREADS), lds, s, rows, ld_rows, d_labels, ld_labels, N, C, M, W,
                       (int)A, n_ctiles, rpc, fe, aligned, d_obs, d_alt, d_miss, d_bad);
  }
  return hipGetLastError();
}

extern "C" int gnx_ancestry_allele_counts_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels,
                                              int64_t ld_labels, int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t* d_n_obs,
                                              int32_t* d_n_alt, int32_t* d_n_miss, int64_t debug_rows_per_chunk, int64_t debug_flush_every) {
  if (!ctx) return GNX_EINVAL;
  int rc = counts_check(ctx, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, debug_rows_per_chunk, debug_flush_every);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  if ((rc = zero_tables(ctx, A, C, d_n_obs, d_n_alt, d_n_miss, s)) != GNX_OK) return rc;
  if (N == 0) return GNX_OK;
  unsigned long long* d_bad;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  HIPCHK(ctx, gnx_launch_allele_counts(d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_n_obs, d_n_alt, d_n_miss,
                                       debug_rows_per_chunk, debug_flush_every, d_bad, ctx->n_cu, s));
  return gnx_sum_read_verdict(ctx, "ancestry_allele_counts", d_bad, A, AC_TAIL, nullptr, s);
}

namespace {
// the (A, C) int32 tables of a host-pointer entry: three slabs of tb bytes in ws_b32, NULL for a table the caller did not ask for
int table_slab(gnx_ctx* ctx, size_t tb, const int32_t* n_obs, const int32_t* n_alt, const int32_t* n_miss, int32_t** d_obs, int32_t** d_alt,
               int32_t** d_miss) {
  const int rc = gnx_ws_reserve(ctx, ctx->ws_b32, 3 * tb);
  if (rc != GNX_OK) return rc;
  char* o = (char*)ctx->ws_b32.p;
  *d_obs = n_obs ? (int32_t*)o : nullptr;
  *d_alt = n_alt ? (int32_t*)(o + tb) : nullptr;
  *d_miss = n_miss ? (int32_t*)(o + 2 * tb) : nullptr;
  return GNX_OK;
}
}  // namespace

extern "C" int gnx_ancestry_allele_counts(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels,
                                          int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t* n_obs, int32_t* n_alt, int32_t* n_miss,
                                          int64_t debug_rows_per_chunk, int64_t debug_flush_every) {
  if (!ctx) return GNX_EINVAL;
  int rc = counts_check(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A, debug_rows_per_chunk, debug_flush_every);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const size_t tb = ((size_t)A * (size_t)C * sizeof(int32_t) + 255) & ~(size_t)255;
  int32_t *d_obs, *d_alt, *d_miss;
  if ((rc = table_slab(ctx, tb, n_obs, n_alt, n_miss, &d_obs, &d_alt, &d_miss)) != GNX_OK) return rc;
  std::string msg;
  if (N > 0 && (rc = gnx_sum_stage_rows_labels(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  rc = gnx_ancestry_allele_counts_dev(ctx, ctx->ws_xu.p, row_kind, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, d_obs, d_alt,
                                      d_miss, debug_rows_per_chunk, debug_flush_every);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the counts of the other labels are still handed over)
  msg = ctx->err;
  const size_t b = (size_t)A * (size_t)C * sizeof(int32_t);
  if (n_obs) HIPCHK(ctx, hipMemcpyAsync(n_obs, d_obs, b, hipMemcpyDeviceToHost, s));
  if (n_alt) HIPCHK(ctx, hipMemcpyAsync(n_alt, d_alt, b, hipMemcpyDeviceToHost, s));
  if (n_miss) HIPCHK(ctx, hipMemcpyAsync(n_miss, d_miss, b, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  ctx->err = msg;
  return rc;
}

namespace {
int dosage_check(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N, int64_t C, int64_t M,
                 int64_t W, int32_t A, int32_t ancestry, const void* dosage, int64_t ld_d, const void* hapcount, int64_t ld_h) {
  int rc = geometry_check(ctx, "ancestry_dosage", rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A);
  if (rc != GNX_OK) return rc;
  if (N & 1) return gnx_fail(ctx, GNX_EINVAL, "ancestry_dosage: N must be even (an individual has two haplotype rows)");
  if (ancestry < 0 || ancestry >= A) return gnx_fail(ctx, GNX_EINVAL, "ancestry_dosage: the ancestry lies outside [0, A)");
  if ((dosage && ld_d < C) || (hapcount && ld_h < C)) return gnx_fail(ctx, GNX_EINVAL, "ancestry_dosage: an output's row stride is smaller than C");
  return GNX_OK;
}
}  // namespace

extern "C" int gnx_ancestry_dosage_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                       int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, uint8_t* d_dosage, int64_t ld_dosage,
                                       uint8_t* d_hapcount, int64_t ld_hapcount) {
  if (!ctx) return GNX_EINVAL;
  int rc = dosage_check(ctx, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, ancestry, d_dosage, ld_dosage, d_hapcount, ld_hapcount);
  if (rc != GNX_OK) return rc;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  unsigned long long* d_bad;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  const int64_t G = (C + AC_COLS - 1) / AC_COLS, total = (N / 2) * G;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)ctx->n_cu * 32));
  const int a_in = gnx_sum_rows_aligned(d_rows, row_kind, ld_rows);
  const int a_out = (!d_dosage || ((uintptr_t)d_dosage % 16 == 0 && ld_dosage % 16 == 0)) &&
                    (!d_hapcount || ((uintptr_t)d_hapcount % 16 == 0 && ld_hapcount % 16 == 0));
  const uint8_t* rows = (const uint8_t*)d_rows;
  if (row_kind == GNX_ROWS_PACKED2)
    hipLaunchKernelGGL(k_ancestry_dosage<GNX_ROWS_PACKED2>, dim3(grid), dim3(256), 0, s, rows, ld_rows, d_labels, ld_labels, N / 2, C, M, W, (int)A,
                       (int)ancestry, G, a_in, d_dosage, ld_dosage, d_hapcount, ld_hapcount, a_out, d_bad);
  else
    hipLaunchKernelGGL(k_ancestry_dosage<GNX_ROWS_INT8>, dim3(grid), dim3(256), 0, s, rows, ld_rows, d_labels, ld_labels, N / 2, C, M, W, (int)A,
                       (int)ancestry, G, a_in, d_dosage, ld_dosage, d_hapcount, ld_hapcount, a_out, d_bad);
  HIPCHK(ctx, hipGetLastError());
  return gnx_sum_read_verdict(ctx, "ancestry_dosage", d_bad, A, AC_TAIL, nullptr, s);
}

extern "C" int gnx_ancestry_dosage(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                                   int64_t C, int64_t M, int64_t W, int32_t A, int32_t ancestry, uint8_t* dosage, int64_t ld_dosage,
                                   uint8_t* hapcount, int64_t ld_hapcount) {
  if (!ctx) return GNX_EINVAL;
  int rc = dosage_check(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A, ancestry, dosage, ld_dosage, hapcount, ld_hapcount);
  if (rc != GNX_OK) return rc;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const int64_t n_ind = N / 2, ldo = (C + 15) / 16 * 16;
  const size_t bo = ((size_t)n_ind * (size_t)ldo + 255) & ~(size_t)255;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b32, 2 * bo)) != GNX_OK) return rc;
  uint8_t* d_d = dosage ? (uint8_t*)ctx->ws_b32.p : nullptr;
  uint8_t* d_h = hapcount ? (uint8_t*)ctx->ws_b32.p + bo : nullptr;
  if ((rc = gnx_sum_stage_rows_labels(ctx, rows, row_kind, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  rc = gnx_ancestry_dosage_dev(ctx, ctx->ws_xu.p, row_kind, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, ancestry, d_d, ldo, d_h,
                               ldo);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  const std::string msg = ctx->err;
  if (dosage)
    HIPCHK(ctx, hipMemcpy2DAsync(dosage, (size_t)ld_dosage, d_d, (size_t)ldo, (size_t)C, (size_t)n_ind, hipMemcpyDeviceToHost, s));
  if (hapcount)
    HIPCHK(ctx, hipMemcpy2DAsync(hapcount, (size_t)ld_hapcount, d_h, (size_t)ldo, (size_t)C, (size_t)n_ind, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  ctx->err = msg;
  return rc;
}

// The file path's form: the packed rows of gnx_infer_gt2's batches (gnx_api_vcf.hip: the same staging, column map, k_gt2_to_p2, row pitch
// and batch size), counted against the caller's labels; the tables live in ws_b32 and leave once, after the last batch.
extern "C" int gnx_ancestry_allele_counts_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src,
                                              const int32_t* labels, int32_t* n_obs, int32_t* n_alt, int32_t* n_miss) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  if (N < 0 || N >= ((int64_t)1 << 31) || V < 0 || ldg < (N + 3) / 4 || !src || (N > 0 && (!labels || (V > 0 && !G))))
    return gnx_fail(ctx, GNX_EINVAL, "ancestry_allele_counts_gt2: bad G / V / ldg / N / src / labels");
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  if (A > AC_MAX_A)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_allele_counts_gt2: A = " + std::to_string(A) + " ancestries, at most " + std::to_string(AC_MAX_A) +
                                               " are counted");
  if (A > ((int64_t)1 << 31) / C) return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_allele_counts_gt2: A * C must stay below 2^31");
  int rc = gnx_sum_check_src(ctx, "ancestry_allele_counts_gt2", src, C, V);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const size_t tbytes = (size_t)A * (size_t)C * sizeof(int32_t), tb = (tbytes + 255) & ~(size_t)255;
  int32_t *d_obs, *d_alt, *d_miss;
  if ((rc = table_slab(ctx, tb, n_obs, n_alt, n_miss, &d_obs, &d_alt, &d_miss)) != GNX_OK) return rc;
  HIPCHK(ctx, hipMemsetAsync(ctx->ws_b32.p, 0, 3 * tb, s));
  unsigned long long h_bad = 0;
  if (N > 0) {
    gnx_sum_gt2 st;
    unsigned long long* d_bad;
    if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, true, &st, s)) != GNX_OK) return rc;
    if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
    for (int64_t n0 = 0; n0 < N; n0 += st.nb) {
      const int64_t n = std::min(st.nb, N - n0);
      HIPCHK(ctx, gnx_sum_gt2_batch(st, n0, n, C, ctx->ws_xu.p, s));
      HIPCHK(ctx, gnx_launch_allele_counts(ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab + n0 * W, W, n, C, M, W, A, d_obs, d_alt, d_miss, 0, 0, d_bad,
                                           ctx->n_cu, s));
    }
    HIPCHK(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  }
  if (n_obs) HIPCHK(ctx, hipMemcpyAsync(n_obs, d_obs, tbytes, hipMemcpyDeviceToHost, s));
  if (n_alt) HIPCHK(ctx, hipMemcpyAsync(n_alt, d_alt, tbytes, hipMemcpyDeviceToHost, s));
  if (n_miss) HIPCHK(ctx, hipMemcpyAsync(n_miss, d_miss, tbytes, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return gnx_sum_label_verdict(ctx, "ancestry_allele_counts_gt2", h_bad, A, AC_TAIL, nullptr);
}
