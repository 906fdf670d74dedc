// summary/gnx_summary_host.h — the host side the ancestry-specific ops of this folder share (k_allele_counts.hip, k_ancestry_assoc.hip,
// k_ancestry_assoc_logit.hip, k_ancestry_score.hip and, through gnx_as_gram.h, k_ancestry_pairs.hip and k_ancestry_ld.hip): the refusals
// on the geometry, the staging of host rows, labels and phenotypes, the file path's staging (gnx_infer_gt2's: gnx_api_vcf.hip keeps its
// own copy), the counter of labels out of range and its verdict.  One definition of each, in gnx_summary_host.hip, which also defines
// the host side of gnx_as_gram.h (what the two Gram ops share beyond this); the device-side row helpers stay in gnx_assoc_rows.h.
#pragma once
#include "gnx_assoc_rows.h"

// ---- the geometry every op refuses on ------------------------------------------------------------------------------------------------------
enum : unsigned {
  GNX_SUM_N_EVEN = 1u,      // an individual has two haplotype rows (every op but the allele counts)
  GNX_SUM_ROWS_BUILT = 2u,  // the rows are built by this call (the _gt2 forms): `rows` is not looked at
  // the op refuses null pointers itself: the two association ops do, whatever N is, in one clause with y, Z and the outputs and under a
  // sentence of their own ("a null pointer (only ... may be NULL)"), which "no rows or no labels" here would pre-empt
  GNX_SUM_OWN_NULLS = 4u,
};
// usable context, row_kind, N / C / A, [N even], M * W <= C, both strides, [no rows or no labels]: GNX_OK or the refusal, "<who>: ..."
int gnx_sum_geometry_check(gnx_ctx* ctx, const char* who, unsigned flags, const void* rows, int row_kind, int64_t ld_rows, const void* labels,
                           int64_t ld_labels, int64_t N, int64_t C, int64_t M, int64_t W, int32_t A);
// the rows' base and stride allow as_fields16's one-load form: multiples of 4 (packed) or 16 (int8) bytes
int gnx_sum_rows_aligned(const void* rows, int row_kind, int64_t ld);

// ---- host-pointer forms --------------------------------------------------------------------------------------------------------------------
// the host rows and labels -> ws_xu and ws_lab (N == 0: the two reserves alone, so that neither pointer is null)
int gnx_sum_stage_rows_labels(gnx_ctx* ctx, const void* rows, int row_kind, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N,
                              int64_t C, int64_t W, hipStream_t s);
// y | Z | use of n_ind individuals -> ws_scale (each part padded to 256 bytes); d_use is NULL where use is
struct gnx_sum_pheno {
  double *d_y, *d_Z;
  uint8_t* d_use;
};
int gnx_sum_stage_pheno(gnx_ctx* ctx, const double* y, const double* Z, int32_t K, const uint8_t* use, int64_t n_ind, gnx_sum_pheno* p, hipStream_t s);
// the many-trait form (k_ancestry_assoc_traits.hip): Y (n_ind, T) with row stride ldy -> compact (n_ind, T) | Z | use in ws_scale
struct gnx_sum_traits {
  double *d_Y, *d_Z;
  uint8_t* d_use;
};
int gnx_sum_stage_traits(gnx_ctx* ctx, const double* Y, int64_t ldy, int32_t T, const double* Z, int32_t K, const uint8_t* use, int64_t n_ind,
                         gnx_sum_traits* p, hipStream_t s);
// room in ws_p64 for what the two prep kernels write: zy (n_ind, K + 1) float64, padded to 256 bytes, then part, a byte per individual
int gnx_sum_zy_part(gnx_ctx* ctx, int64_t n_ind, int32_t K, double** zy, uint8_t** part);

// ---- the file path's forms (_gt2) ----------------------------------------------------------------------------------------------------------
struct gnx_sum_gt2 {
  int64_t ldp, nb, ldg_d, V;  // pitch of a packed row (64-byte aligned); haplotypes per batch (a multiple of 4); pitch of G on the device
  const uint8_t* d_G;         // ws_gt2
  const int32_t *d_src, *d_lab;  // ws_src; ws_lab: (N, W), compact
};
// GNX_EINVAL "<who>: bad G / V / ldg / N / src", and "<who>: column map entry outside the variant rows"
int gnx_sum_gt2_args(gnx_ctx* ctx, const char* who, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src);
int gnx_sum_check_src(gnx_ctx* ctx, const char* who, const int32_t* src, int64_t C, int64_t V);
// ldp, nb and ldg_d: functions of (C, N, ldg, GNX_HOST_BATCH) alone
void gnx_sum_gt2_sizes(const gnx_ctx* ctx, int64_t C, int64_t ldg, int64_t N, gnx_sum_gt2* st);
// sizes, the reserves of ws_gt2, ws_src, ws_lab (and ws_xu for one batch of packed rows where batch_rows), and for N > 0 the uploads of src, G
// and the labels.  Arguments checked by the caller.
int gnx_sum_gt2_stage(gnx_ctx* ctx, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src, const int32_t* labels, int64_t C,
                      int64_t W, bool batch_rows, gnx_sum_gt2* st, hipStream_t s);
// the packed rows of the haplotypes n0 .. n0 + n - 1 (n0 a multiple of nb) -> dst; all N rows -> dst, batch by batch (dst: N rows of ldp bytes)
hipError_t gnx_sum_gt2_batch(const gnx_sum_gt2& st, int64_t n0, int64_t n, int64_t C, void* dst, hipStream_t s);
hipError_t gnx_sum_gt2_all_rows(const gnx_sum_gt2& st, int64_t N, int64_t C, void* dst, hipStream_t s);

// ---- labels outside [0, A) -----------------------------------------------------------------------------------------------------------------
// the counter: 256 bytes of ws_misc, its first `slots` words zeroed on the stream
int gnx_sum_bad_counter(gnx_ctx* ctx, int slots, unsigned long long** d_bad, hipStream_t s);
// *n_bad = h_bad (where n_bad is not NULL); GNX_OK, or GNX_EINVAL "<who>: <h_bad> labels lie outside [0, <A>); <tail>"
int gnx_sum_label_verdict(gnx_ctx* ctx, const char* who, unsigned long long h_bad, int32_t A, const char* tail, int64_t* n_bad);
// reads the counter back (one synchronisation of the stream), then the verdict
int gnx_sum_read_verdict(gnx_ctx* ctx, const char* who, const unsigned long long* d_bad, int32_t A, const char* tail, int64_t* n_bad, hipStream_t s);
