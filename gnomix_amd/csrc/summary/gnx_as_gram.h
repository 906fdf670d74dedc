// summary/gnx_as_gram.h — the int8 Gram core under k_ancestry_pairs.hip and k_ancestry_ld.hip: both stage the masked bytes d and o of two
// tiles of 64 rows in LDS, chunk by chunk of the contracted index, and form D_I D_J^T, D_I O_J^T, O_I D_J^T and O_I O_J^T of them on the
// matrix cores; pairs contracts over SNPs (rows = individuals), LD over haplotypes (rows = SNPs).  Here: the tile constants, the product
// step, the accumulators' (row, column), the put, and the host side the two share (the split, the common refusals, the label count, the
// tables of a host-pointer form and the three forms of an entry point).  What is no template is defined in gnx_summary_host.hip.
//  * Products.  Wave v owns rows 16 v .. 16 v + 15 of tile I and all four 16-column tiles of J: 16 accumulators of four int32 each, two
//    v_mfma_i32_16x16x64_i8 steps per chunk.  Both operands are 16 consecutive bytes of a staged row (A: row = lane & 15 of the wave's
//    rows, B: row = lane & 15 of the column tile, k-block = lane >> 4), the layout of k_lda_gram and k_knn_argmin; C/D: column =
//    lane & 15, row = 4 (lane >> 4) + reg.
//  * LDS pitch 160 bytes (GRAM_KC + 32), the read side.  The hardware serves a 16-byte read of a wave in four groups of 16 lanes, and a
//    group is not 16 consecutive lanes: it holds every row r = lane & 15 once, the rows 0-3 and 12-15 with one k-block q and the rows
//    4-11 with q + 1 (or the other way round).  In units of the 16-byte slot, 16 of which make the 64 banks, row r and k-block q sit at
//    10 r + q: 10 r mod 16 = 2 (5 r mod 8) takes each even value twice, for r and r + 8, and exactly one of r and r + 8 lies in 4..11,
//    so the + 1 of that one makes the 16 slots of a group distinct: conflict-free, for both k-steps (+ 4 slots for all lanes).  An
//    80-byte pitch (slot 5 r + q) is conflict-free only if a group were 16 consecutive lanes.  (The grouping is taken from measurements
//    of this chip that are public; the counter SQ_LDS_BANK_CONFLICT has not been read on either kernel.)  Each kernel argues its own
//    store side.
//  * The split.  Few tile pairs do not fill the chip, so the contracted index is cut into segments of whole chunks and grid = pairs x
//    segments.  The segments' sums are combined with int32 vector atomic adds (global_atomic_add, no return value) into tables zeroed
//    first: integer addition is associative, so the order cannot change a sum.  Chosen over a workspace plus a reduce kernel because that
//    costs segments x the tables written and read again and one more launch, where the atomics touch each element once per segment, and a
//    segment is at least min_chunks chunks of MFMA work per element.  One segment (many tile pairs) uses plain stores.
#pragma once
#include "gnx_summary_host.h"

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int GRAM_T = 64;                   // rows per tile
constexpr int GRAM_KC = 128;                 // contracted indices per chunk: two steps of the MFMA's K = 64
constexpr int GRAM_P = GRAM_KC + 32;         // LDS row pitch, bytes
constexpr int GRAM_IMG = GRAM_T * GRAM_P;    // bytes of one staged image; tz holds four: d of tile I, o of tile I, d of tile J, o of tile J

// ---- device side ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gram_zero(v4i (&dd)[4], v4i (&dx)[4], v4i (&xd)[4], v4i (&oo)[4]) {
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) dd[jt] = dx[jt] = xd[jt] = oo[jt] = v4i{0, 0, 0, 0};
}

// A lane of wave wv is (lr, lq) = (lane & 15, lane >> 4): the row and the k-block of its operands, the column and the row quad of its results.
// Its operand bytes of a chunk, as offsets into tz: A from the d image of tile I, B from the d image at b_img (2 GRAM_IMG: tile J; 0: a
// diagonal pair that staged its tile once).
__device__ __forceinline__ int gram_a_off(int wv, int lr, int lq) { return (wv * 16 + lr) * GRAM_P + lq * 16; }
__device__ __forceinline__ int gram_b_off(int b_img, int lr, int lq) { return b_img + lr * GRAM_P + lq * 16; }

// one staged chunk: dd += D_I D_J^T, dx += D_I O_J^T, oo += O_I O_J^T and, where with_xd (block-uniform), xd += O_I D_J^T
__device__ __forceinline__ void gram_chunk(const uint8_t* ap, const uint8_t* bp, bool with_xd, v4i (&dd)[4], v4i (&dx)[4], v4i (&xd)[4], v4i (&oo)[4]) {
#pragma unroll
  for (int ks = 0; ks < GRAM_KC / 64; ++ks) {
    const v4i ad = *reinterpret_cast<const v4i*>(ap + 64 * ks);
    const v4i ao = *reinterpret_cast<const v4i*>(ap + GRAM_IMG + 64 * ks);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const v4i bd = *reinterpret_cast<const v4i*>(bp + jt * 16 * GRAM_P + 64 * ks);
      const v4i bo = *reinterpret_cast<const v4i*>(bp + GRAM_IMG + jt * 16 * GRAM_P + 64 * ks);
      dd[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bd, dd[jt], 0, 0, 0);
      dx[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bo, dx[jt], 0, 0, 0);
      oo[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bo, oo[jt], 0, 0, 0);
      if (with_xd) xd[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bd, xd[jt], 0, 0, 0);
    }
  }
}

// element r of accumulator jt: its row and its column, from the first row of tile I and the first column of tile J
__device__ __forceinline__ int64_t gram_row(int64_t i0, int wv, int lq, int r) { return i0 + wv * 16 + 4 * lq + r; }
__device__ __forceinline__ int64_t gram_col(int64_t j0, int lr, int jt) { return j0 + jt * 16 + lr; }

__device__ __forceinline__ void gram_put(int32_t* __restrict__ T, size_t at, int32_t v, int atomic) {
  if (atomic) atomicAdd(T + at, v);
  else T[at] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
extern const char* const GNX_GRAM_TAIL;   // the label verdict's sentence

// chunks per segment and the number of segments, a function of its arguments alone: about four workgroups per CU where the pairs are
// fewer, no segment below min_chunks; dbg > 0 (the tests): segments of dbg contracted indices, rounded up to chunks
void gnx_gram_split(int64_t chunks, int64_t pairs, int n_cu, int64_t dbg, int64_t min_chunks, int64_t* cpb, int64_t* nseg);
// GNX_EUNSUPPORTED "<who>: <pairs> tile pairs x <nseg> <what> segments exceed one grid"
int gnx_gram_grid_check(gnx_ctx* ctx, const char* who, int64_t pairs, int64_t nseg, const char* what);
// the labels outside [0, A) among the rows' windows [k0, k1), ADDED to *d_bad (k_ancestry_gram_labels)
int gnx_gram_count_labels(gnx_ctx* ctx, const int32_t* d_labels, int64_t ld_labels, int64_t N, int64_t k0, int64_t k1, int32_t A,
                          unsigned long long* d_bad, hipStream_t s);
// the rows [r0, r0 + rows) x cols of every table that is not NULL <- 0
int gnx_gram_zero(gnx_ctx* ctx, int32_t* const tabs[], int n_tabs, int64_t ld, int64_t r0, int64_t rows, int64_t cols, hipStream_t s);

struct gnx_gram_rows {   // the rows and labels of a call, on the host or on the device
  const void* rows;
  int row_kind;
  int64_t ld_rows;
  const int32_t* labels;
  int64_t ld_labels;
};
struct gnx_gram_call {   // what an entry point hands its form
  const char* who;
  int64_t N, C, M, W;
  int32_t A, ancestry;
  int64_t c0, c1;
  int n_tabs;            // the caller's tables (any may be NULL), their row stride, and the (rows, cols) of each
  int32_t* tabs[4];
  int64_t ld, t_rows, t_cols;
  int64_t* n_bad;
};
// the clauses both checks share, in two runs with the op's own between and behind them.  _range: the geometry (flags:
// gnx_sum_geometry_check's), ancestry, c0 / c1.  _sizes: N < 2^31, debug >= 0, A <= GNX_ALLELE_MAX_A.
int gnx_gram_check_range(gnx_ctx* ctx, const gnx_gram_call& c, unsigned flags, const gnx_gram_rows& R);
int gnx_gram_check_sizes(gnx_ctx* ctx, const gnx_gram_call& c, int64_t dbg);
// a host-pointer form's tables: compact (t_rows, t_cols) slabs in ws_b32, NULL for a table the caller did not ask for; and the slabs
// and the count -> the host, one synchronisation
int gnx_gram_tabs_reserve(gnx_ctx* ctx, const gnx_gram_call& c, int32_t* dev[4]);
int gnx_gram_tabs_copy_out(gnx_ctx* ctx, const gnx_gram_call& c, int32_t* const dev[4], const unsigned long long* d_bad, unsigned long long* h_bad,
                           hipStream_t s);

// The three forms of an entry point, over an op: a struct with the call, c, and the two steps that are the op's own.
// op.check(ctx, built, R, dbg): every refusal that needs no device memory (built: the rows are built by this call).
// op.run(ctx, R, tabs, ld, dbg, d_bad, s): the tables of N > 0 device rows, the labels out of range ADDED to *d_bad.
template <class Op>
int gnx_gram_form_dev(gnx_ctx* ctx, const Op& op, const gnx_gram_rows& R, int64_t dbg) {
  const gnx_gram_call& c = op.c;
  int rc = op.check(ctx, false, R, dbg);
  if (rc != GNX_OK) return rc;
  if (c.n_bad) *c.n_bad = 0;
  if (c.N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  unsigned long long* d_bad;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = op.run(ctx, R, c.tabs, c.ld, dbg, d_bad, s)) != GNX_OK) return rc;
  return gnx_sum_read_verdict(ctx, c.who, d_bad, c.A, GNX_GRAM_TAIL, c.n_bad, s);
}

template <class Op>
int gnx_gram_form_host(gnx_ctx* ctx, const Op& op, const gnx_gram_rows& R, int64_t dbg) {
  const gnx_gram_call& c = op.c;
  int rc = op.check(ctx, false, R, dbg);
  if (rc != GNX_OK) return rc;
  if (c.n_bad) *c.n_bad = 0;
  if (c.N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  int32_t* dev[4];
  unsigned long long *d_bad, h_bad = 0;
  if ((rc = gnx_sum_stage_rows_labels(ctx, R.rows, R.row_kind, R.ld_rows, R.labels, R.ld_labels, c.N, c.C, c.W, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if ((rc = gnx_gram_tabs_reserve(ctx, c, dev)) != GNX_OK) return rc;
  const gnx_gram_rows D{ctx->ws_xu.p, R.row_kind, R.ld_rows, (const int32_t*)ctx->ws_lab.p, R.ld_labels};
  if ((rc = op.run(ctx, D, dev, c.t_cols, dbg, d_bad, s)) != GNX_OK) return rc;
  if ((rc = gnx_gram_tabs_copy_out(ctx, c, dev, d_bad, &h_bad, s)) != GNX_OK) return rc;
  // (GNX_EINVAL here = labels out of range: the tables stand and were handed over)
  return gnx_sum_label_verdict(ctx, c.who, h_bad, c.A, GNX_GRAM_TAIL, c.n_bad);
}

// The file path's form.  Both ops need every row at once, so the WHOLE packed matrix is built in HBM, in device memory of this call's
// own (N rows of gnx_sum_gt2's pitch, freed on return), batch by batch with gnx_infer_gt2's staging; the kernel then runs once.
template <class Op>
int gnx_gram_form_gt2(gnx_ctx* ctx, const Op& op, const uint8_t* G, int64_t V, int64_t ldg, const int32_t* src, const int32_t* labels) {
  const gnx_gram_call& c = op.c;
  const std::string w(c.who);
  int rc = gnx_sum_gt2_args(ctx, c.who, G, V, ldg, c.N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = op.check(ctx, true, gnx_gram_rows{nullptr, GNX_ROWS_PACKED2, (c.C + 3) / 4, labels, c.W}, 0)) != GNX_OK) return rc;
  if ((rc = gnx_sum_check_src(ctx, c.who, src, c.C, V)) != GNX_OK) return rc;
  if (c.n_bad) *c.n_bad = 0;
  if (c.N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  gnx_sum_gt2 st;
  gnx_sum_gt2_sizes(ctx, c.C, ldg, c.N, &st);
  {
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t need = (size_t)c.N * st.ldp + (size_t)V * st.ldg_d + (size_t)c.n_tabs * (size_t)c.t_rows * (size_t)c.t_cols * 4 + (size_t)c.N * c.W * 4 +
                        (size_t)c.C * 4;
    if (need > total_b)
      return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": the packed rows of " + std::to_string(c.N) + " haplotypes plus the tables take " + std::to_string(need) +
                                                 " bytes, the device has " + std::to_string(total_b));
  }
  int32_t* dev[4];
  gnx_dev_tmp P;
  unsigned long long *d_bad, h_bad = 0;
  if ((rc = gnx_gram_tabs_reserve(ctx, c, dev)) != GNX_OK) return rc;
  if (P.alloc((size_t)c.N * st.ldp + 256) != hipSuccess)   // (before anything is enqueued)
    return gnx_fail(ctx, GNX_ENOMEM, w + ": no device memory for " + std::to_string((size_t)c.N * st.ldp) + " bytes of packed rows");
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, c.N, src, labels, c.C, c.W, false, &st, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  HIPCHK(ctx, gnx_sum_gt2_all_rows(st, c.N, c.C, P.p, s));
  rc = op.run(ctx, gnx_gram_rows{P.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab, c.W}, dev, c.t_cols, 0, d_bad, s);
  if (rc == GNX_OK) rc = gnx_gram_tabs_copy_out(ctx, c, dev, d_bad, &h_bad, s);
  else (void)hipStreamSynchronize(s);   // the rows are freed on return: nothing may still read them
  if (rc != GNX_OK) return rc;
  return gnx_sum_label_verdict(ctx, c.who, h_bad, c.A, GNX_GRAM_TAIL, c.n_bad);
}
