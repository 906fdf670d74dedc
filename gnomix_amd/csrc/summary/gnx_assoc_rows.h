// summary/gnx_assoc_rows.h — what the two ancestry-specific association files share about rows and windows (k_ancestry_assoc.hip, the
// linear model's sufficient statistics; k_ancestry_assoc_logit.hip, the logistic fits): one definition of each.
#pragma once
#include "../gnx_internal.h"

// the field of column c of one row: 0 REF, 1 ALT, 2 / 3 missing (the coding of k_allele_counts.hip's load_fields)
template <int KIND>
__device__ __forceinline__ uint32_t as_code(const uint8_t* __restrict__ row, int64_t c) {
  if (KIND == GNX_ROWS_PACKED2) return ((uint32_t)row[c >> 2] >> (2 * (int)(c & 3))) & 3u;
  const uint32_t b = row[c];
  return b <= 1u ? b : 2u;
}

inline int64_t as_min_row_bytes(int row_kind, int64_t C) { return row_kind == GNX_ROWS_PACKED2 ? (C + 3) / 4 : C; }

inline int64_t as_win(int64_t c, int64_t M, int64_t W) { return std::min(c / M, W - 1); }
