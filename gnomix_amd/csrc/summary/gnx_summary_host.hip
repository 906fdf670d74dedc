// summary/gnx_summary_host.hip — the only definitions of what gnx_summary_host.h declares and of the host side of gnx_as_gram.h.  Host code
// but for one kernel: k_ancestry_gram_labels, the label count of the two Gram ops.
#include "gnx_as_gram.h"

int gnx_sum_geometry_check(gnx_ctx* ctx, const char* who, unsigned flags, const void* rows, int row_kind, int64_t ld_rows, const void* labels,
                           int64_t ld_labels, int64_t N, int64_t C, int64_t M, int64_t W, int32_t A) {
  const std::string w(who);
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (row_kind != GNX_ROWS_INT8 && row_kind != GNX_ROWS_PACKED2) return gnx_fail(ctx, GNX_EINVAL, w + ": row_kind is GNX_ROWS_INT8 or GNX_ROWS_PACKED2");
  if (N < 0 || C < 1 || A < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need N >= 0, C >= 1 and A >= 1");
  if ((flags & GNX_SUM_N_EVEN) && (N & 1)) return gnx_fail(ctx, GNX_EINVAL, w + ": N must be even (an individual has two haplotype rows)");
  if (M < 1 || W < 1 || M > C || W > C / M) return gnx_fail(ctx, GNX_EINVAL, w + ": need M >= 1, W >= 1 and M * W <= C");
  if (ld_rows < as_min_row_bytes(row_kind, C)) return gnx_fail(ctx, GNX_EINVAL, w + ": the rows' stride is smaller than a row (C bytes, or ceil(C / 4) packed)");
  if (ld_labels < W) return gnx_fail(ctx, GNX_EINVAL, w + ": the labels' row stride is smaller than W");
  if (flags & GNX_SUM_OWN_NULLS) return GNX_OK;
  const bool rows_missing = !(flags & GNX_SUM_ROWS_BUILT) && !rows;
  if (N > 0 && (rows_missing || !labels)) return gnx_fail(ctx, GNX_EINVAL, w + ": no rows or no labels");
  return GNX_OK;
}

int gnx_sum_rows_aligned(const void* rows, int row_kind, int64_t ld) {
  const uintptr_t a = row_kind == GNX_ROWS_PACKED2 ? 4 : 16;
  return ((uintptr_t)rows % a == 0) && (ld % (int64_t)a == 0);
}

int gnx_sum_stage_rows_labels(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                              int64_t C, int64_t W, hipStream_t s) {
  // the last row ends after its own bytes / labels, not after a whole stride
  const size_t br = N > 0 ? (size_t)(N - 1) * (size_t)ld_rows + (size_t)as_min_row_bytes(row_kind, C) : 0;
  const size_t bl = N > 0 ? ((size_t)(N - 1) * (size_t)ld_labels + (size_t)W) * sizeof(int32_t) : 0;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_xu, br + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, bl + 64)) != GNX_OK) return rc;
  if (N > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_xu.p, rows, br, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, labels, bl, hipMemcpyHostToDevice, s));
  }
  return GNX_OK;
}

int gnx_sum_stage_pheno(gnx_ctx* ctx, const double* y, const double* Z, int32_t K, const uint8_t* use, int64_t n_ind, gnx_sum_pheno* p, hipStream_t s) {
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t by = up((size_t)n_ind * 8), bz = up((size_t)n_ind * K * 8), bu = up((size_t)n_ind);
  const int rc = gnx_ws_reserve(ctx, ctx->ws_scale, by + bz + bu + 64);
  if (rc != GNX_OK) return rc;
  char* sc = (char*)ctx->ws_scale.p;
  p->d_y = (double*)sc;
  p->d_Z = (double*)(sc + by);
  p->d_use = use ? (uint8_t*)(sc + by + bz) : nullptr;
  if (n_ind > 0) {
    HIPCHK(ctx, hipMemcpyAsync(p->d_y, y, (size_t)n_ind * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(p->d_Z, Z, (size_t)n_ind * K * 8, hipMemcpyHostToDevice, s));
    if (use) HIPCHK(ctx, hipMemcpyAsync(p->d_use, use, (size_t)n_ind, hipMemcpyHostToDevice, s));
  }
  return GNX_OK;
}

int gnx_sum_stage_traits(gnx_ctx* ctx, const double* Y, int64_t ldy, int32_t T, const double* Z, int32_t K, const uint8_t* use, int64_t n_ind,
                         gnx_sum_traits* p, hipStream_t s) {
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t by = up((size_t)n_ind * T * 8), bz = up((size_t)n_ind * K * 8), bu = up((size_t)n_ind);
  const int rc = gnx_ws_reserve(ctx, ctx->ws_scale, by + bz + bu + 64);
  if (rc != GNX_OK) return rc;
  char* sc = (char*)ctx->ws_scale.p;
  p->d_Y = (double*)sc;
  p->d_Z = (double*)(sc + by);
  p->d_use = use ? (uint8_t*)(sc + by + bz) : nullptr;
  if (n_ind > 0) {
    HIPCHK(ctx, hipMemcpy2DAsync(p->d_Y, (size_t)T * 8, Y, (size_t)ldy * 8, (size_t)T * 8, (size_t)n_ind, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(p->d_Z, Z, (size_t)n_ind * K * 8, hipMemcpyHostToDevice, s));
    if (use) HIPCHK(ctx, hipMemcpyAsync(p->d_use, use, (size_t)n_ind, hipMemcpyHostToDevice, s));
  }
  return GNX_OK;
}

int gnx_sum_zy_part(gnx_ctx* ctx, int64_t n_ind, int32_t K, double** zy, uint8_t** part) {
  const size_t zy_bytes = (((size_t)n_ind * (K + 1) * sizeof(double)) + 255) & ~(size_t)255;
  const int rc = gnx_ws_reserve(ctx, ctx->ws_p64, zy_bytes + (size_t)n_ind + 256);
  if (rc != GNX_OK) return rc;
  *zy = (double*)ctx->ws_p64.p;
  *part = (uint8_t*)ctx->ws_p64.p + zy_bytes;
  return GNX_OK;
}

int gnx_sum_gt2_args(gnx_ctx* ctx, const char* who, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src) {
  if (N < 0 || V < 0 || ldg < (N + 3) / 4 || !src || (N > 0 && V > 0 && !G))
    return gnx_fail(ctx, GNX_EINVAL, std::string(who) + ": bad G / V / ldg / N / src");
  return GNX_OK;
}

int gnx_sum_check_src(gnx_ctx* ctx, const char* who, const int32_t* src, int64_t C, int64_t V) {
  for (int64_t c = 0; c < C; ++c) {
    const int32_t sv = src[c];   // -1: a model SNP the query lacks; else the variant row in bits 0 .. 29, the REF flip in bit 30
    if (sv != -1 && (sv < 0 || (int64_t)(sv & 0x3FFFFFFF) >= V))
      return gnx_fail(ctx, GNX_EINVAL, std::string(who) + ": column map entry outside the variant rows");
  }
  return GNX_OK;
}

void gnx_sum_gt2_sizes(const gnx_ctx* ctx, int64_t C, int64_t ldg, int64_t N, gnx_sum_gt2* st) {
  st->ldp = (C + 255) / 256 * 64;
  int64_t nb = (((int64_t)1 << 30) / st->ldp) / 1024 * 1024;  // a batch: <= ~1 GiB of packed rows, whole 1024-haplotype tiles of the transpose
  if (ctx->tune.host_batch > 0) nb = (ctx->tune.host_batch + 3) / 4 * 4;  // tests: several batches on small inputs
  st->nb = std::min(std::max<int64_t>(4, nb), (N + 3) / 4 * 4);
  const int64_t wbytes = (N + 3) / 4;
  st->ldg_d = wbytes == ldg ? ldg : (wbytes + 63) / 64 * 64;
}

int gnx_sum_gt2_stage(gnx_ctx* ctx, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels, int64_t C,
                      int64_t W, bool batch_rows, gnx_sum_gt2* st, hipStream_t s) {
  gnx_sum_gt2_sizes(ctx, C, ldg, N, st);
  const size_t lab_bytes = (size_t)N * (size_t)W * 4;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_gt2, (size_t)V * st->ldg_d + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_src, (size_t)C * 4 + 64)) != GNX_OK) return rc;
  if (batch_rows && (rc = gnx_ws_reserve(ctx, ctx->ws_xu, (size_t)st->nb * st->ldp + 256)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, lab_bytes + 64)) != GNX_OK) return rc;
  st->V = V;
  st->d_G = (const uint8_t*)ctx->ws_gt2.p;
  st->d_src = (const int32_t*)ctx->ws_src.p;
  st->d_lab = (const int32_t*)ctx->ws_lab.p;
  if (N <= 0) return GNX_OK;
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_src.p, src, (size_t)C * 4, hipMemcpyHostToDevice, s));
  if (V > 0) {
    if (st->ldg_d == ldg) HIPCHK(ctx, hipMemcpyAsync(ctx->ws_gt2.p, G, (size_t)V * ldg, hipMemcpyHostToDevice, s));
    else HIPCHK(ctx, hipMemcpy2DAsync(ctx->ws_gt2.p, (size_t)st->ldg_d, G, (size_t)ldg, (size_t)((N + 3) / 4), (size_t)V, hipMemcpyHostToDevice, s));
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, labels, lab_bytes, hipMemcpyHostToDevice, s));
  return GNX_OK;
}

hipError_t gnx_sum_gt2_batch(const gnx_sum_gt2& st, int64_t n0, int64_t n, int64_t C, void* dst, hipStream_t s) {
  return gnx_launch_gt2_to_p2(st.d_G, st.V, st.ldg_d, n0, n, st.d_src, C, (uint8_t*)dst, st.ldp, s);
}

// k_gt2_to_p2 (k_gt2.hip) writes the rows h < n of its batch and no others (its store loop breaks at h >= N), and of a row only the bytes
// below ldp: a launch's last tile of 1024 haplotypes is not written whole.  So dst needs N rows of ldp bytes, without padding to a batch,
// a tile or a multiple of four.
hipError_t gnx_sum_gt2_all_rows(const gnx_sum_gt2& st, int64_t N, int64_t C, void* dst, hipStream_t s) {
  for (int64_t n0 = 0; n0 < N; n0 += st.nb)
    GNX_HIPRET(gnx_sum_gt2_batch(st, n0, std::min(st.nb, N - n0), C, (uint8_t*)dst + (size_t)n0 * st.ldp, s));
  return hipSuccess;
}

int gnx_sum_bad_counter(gnx_ctx* ctx, int slots, unsigned long long** d_bad, hipStream_t s) {
  const int rc = gnx_ws_reserve(ctx, ctx->ws_misc, 256);
  if (rc != GNX_OK) return rc;
  *d_bad = (unsigned long long*)ctx->ws_misc.p;
  HIPCHK(ctx, hipMemsetAsync(*d_bad, 0, (size_t)slots * sizeof(unsigned long long), s));
  return GNX_OK;
}

int gnx_sum_label_verdict(gnx_ctx* ctx, const char* who, unsigned long long h_bad, int32_t A, const char* tail, int64_t* n_bad) {
  if (n_bad) *n_bad = (int64_t)h_bad;
  if (h_bad)
    return gnx_fail(ctx, GNX_EINVAL, std::string(who) + ": " + std::to_string(h_bad) + " labels lie outside [0, " + std::to_string(A) + "); " + tail);
  return GNX_OK;
}

int gnx_sum_read_verdict(gnx_ctx* ctx, const char* who, const unsigned long long* d_bad, int32_t A, const char* tail, int64_t* n_bad, hipStream_t s) {
  unsigned long long h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return gnx_sum_label_verdict(ctx, who, h_bad, A, tail, n_bad);
}

// ---- the host side of gnx_as_gram.h --------------------------------------------------------------------------------------------------------
const char* const GNX_GRAM_TAIL = "such a haplotype counts for no ancestry at that window";

void gnx_gram_split(int64_t chunks, int64_t pairs, int n_cu, int64_t dbg, int64_t min_chunks, int64_t* cpb, int64_t* nseg) {
  int64_t per = chunks;
  if (dbg > 0) {
    per = (dbg + GRAM_KC - 1) / GRAM_KC;
  } else {
    const int64_t want = (int64_t)n_cu * 4;            // about four workgroups per CU
    if (pairs < want) {
      const int64_t ns = (want + pairs - 1) / pairs;   // segments that would fill the chip
      per = std::max(min_chunks, (chunks + ns - 1) / ns);
    }
  }
  per = std::min(per, chunks);
  *cpb = per;
  *nseg = (chunks + per - 1) / per;
}

int gnx_gram_grid_check(gnx_ctx* ctx, const char* who, int64_t pairs, int64_t nseg, const char* what) {
  if (nseg > (((int64_t)1 << 31) - 1) / pairs)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, std::string(who) + ": " + std::to_string(pairs) + " tile pairs x " + std::to_string(nseg) + " " + what +
                                               " segments exceed one grid");
  return GNX_OK;
}

namespace {
// labels outside [0, A) among the rows' windows [k0, k1)
__global__ __launch_bounds__(256) void k_ancestry_gram_labels(const int32_t* __restrict__ lab, int64_t ldl, int64_t N, int64_t k0, int64_t k1, int A,
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
}  // namespace

int gnx_gram_count_labels(gnx_ctx* ctx, const int32_t* d_labels, int64_t ld_labels, int64_t N, int64_t k0, int64_t k1, int32_t A,
                          unsigned long long* d_bad, hipStream_t s) {
  const int64_t total = N * (k1 - k0);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)ctx->n_cu * 8));
  hipLaunchKernelGGL(k_ancestry_gram_labels, dim3(grid), dim3(256), 0, s, d_labels, ld_labels, N, k0, k1, (int)A, d_bad);
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

int gnx_gram_zero(gnx_ctx* ctx, int32_t* const tabs[], int n_tabs, int64_t ld, int64_t r0, int64_t rows, int64_t cols, hipStream_t s) {
  for (int q = 0; q < n_tabs; ++q)
    if (tabs[q]) HIPCHK(ctx, hipMemset2DAsync(tabs[q] + (size_t)r0 * (size_t)ld, (size_t)ld * 4, 0, (size_t)cols * 4, (size_t)rows, s));
  return GNX_OK;
}

int gnx_gram_check_range(gnx_ctx* ctx, const gnx_gram_call& c, unsigned flags, const gnx_gram_rows& R) {
  const std::string w(c.who);
  const int rc = gnx_sum_geometry_check(ctx, c.who, flags, R.rows, R.row_kind, R.ld_rows, R.labels, R.ld_labels, c.N, c.C, c.M, c.W, c.A);
  if (rc != GNX_OK) return rc;
  if (c.ancestry < 0 || c.ancestry >= c.A) return gnx_fail(ctx, GNX_EINVAL, w + ": ancestry outside [0, A)");
  if (c.c0 < 0 || c.c1 <= c.c0 || c.c1 > c.C) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= c0 < c1 <= C");
  return GNX_OK;
}

int gnx_gram_check_sizes(gnx_ctx* ctx, const gnx_gram_call& c, int64_t dbg) {
  const std::string w(c.who);
  if (c.N >= ((int64_t)1 << 31)) return gnx_fail(ctx, GNX_EINVAL, w + ": N must be below 2^31");
  if (dbg < 0) return gnx_fail(ctx, GNX_EINVAL, w + ": the debug argument must be >= 0 (0 = the built-in choice)");
  if (c.A > GNX_ALLELE_MAX_A)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(c.A) + " ancestries, at most " + std::to_string(GNX_ALLELE_MAX_A));
  return GNX_OK;
}

int gnx_gram_tabs_reserve(gnx_ctx* ctx, const gnx_gram_call& c, int32_t* dev[4]) {
  const size_t tb = (((size_t)c.t_rows * (size_t)c.t_cols * 4) + 255) & ~(size_t)255;
  const int rc = gnx_ws_reserve(ctx, ctx->ws_b32, (size_t)c.n_tabs * tb + 64);
  if (rc != GNX_OK) return rc;
  char* o = (char*)ctx->ws_b32.p;
  for (int q = 0; q < c.n_tabs; ++q) dev[q] = c.tabs[q] ? (int32_t*)(o + q * tb) : nullptr;
  return GNX_OK;
}

int gnx_gram_tabs_copy_out(gnx_ctx* ctx, const gnx_gram_call& c, int32_t* const dev[4], const unsigned long long* d_bad, unsigned long long* h_bad,
                           hipStream_t s) {
  const size_t wb = (size_t)c.t_cols * 4;
  for (int q = 0; q < c.n_tabs; ++q)
    if (c.tabs[q]) HIPCHK(ctx, hipMemcpy2DAsync(c.tabs[q], (size_t)c.ld * 4, dev[q], wb, wb, (size_t)c.t_rows, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(h_bad, d_bad, sizeof *h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}
