// summary/gnx_assoc_rows.h — what the files of this folder share about rows and windows (k_ancestry_assoc.hip, the linear model's
// sufficient statistics; k_ancestry_assoc_logit.hip, the logistic fits; k_allele_counts.hip, k_ancestry_score.hip and, through
// gnx_as_gram.h, k_ancestry_pairs.hip and k_ancestry_ld.hip, which read a row 16 columns at a time): one definition of each.
#pragma once
#include "../gnx_internal.h"

// the field of column c of one row: 0 REF, 1 ALT, 2 / 3 missing (the coding of as_fields16 below)
template <int KIND>
__device__ __forceinline__ uint32_t as_code(const uint8_t* __restrict__ row, int64_t c) {
  if (KIND == GNX_ROWS_PACKED2) return ((uint32_t)row[c >> 2] >> (2 * (int)(c & 3))) & 3u;
  const uint32_t b = row[c];
  return b <= 1u ? b : 2u;
}

// the 16 fields of the columns c0 .. c0 + 15 of one row (c0 a multiple of 16), field j at bits 2 j; fields of columns >= C are
// unspecified.  aligned: the rows' base and stride are multiples of 4 (packed) or 16 (int8) bytes, so the group is one load.  Shared by
// k_allele_counts.hip and k_ancestry_score.hip.
template <int KIND>
__device__ __forceinline__ uint32_t as_fields16(const uint8_t* __restrict__ row, int64_t c0, int64_t C, int aligned) {
  if (KIND == GNX_ROWS_PACKED2) {
    const int64_t b0 = c0 >> 2, nbytes = ((C + 3) >> 2) - b0;  // never read past the row's last packed byte
    if (aligned && nbytes >= 4) return *reinterpret_cast<const uint32_t*>(row + b0);
    uint32_t w = 0;
    for (int b = 0; b < 4 && b < nbytes; ++b) w |= (uint32_t)row[b0 + b] << (8 * b);
    return w;
  } else {
    uint32_t x0 = 0x02020202u, x1 = 0x02020202u, x2 = 0x02020202u, x3 = 0x02020202u;
    if (aligned && c0 + 16 <= C) {
      const uint4 q = *reinterpret_cast<const uint4*>(row + c0);
      x0 = q.x; x1 = q.y; x2 = q.z; x3 = q.w;
    } else {
      const int n = (int)((C - c0 < 16) ? C - c0 : 16);
      uint32_t y0 = 0, y1 = 0, y2 = 0, y3 = 0;
      for (int j = 0; j < n; ++j) {
        const uint32_t b = (uint32_t)row[c0 + j] << (8 * (j & 3));
        if (j < 4) y0 |= b; else if (j < 8) y1 |= b; else if (j < 12) y2 |= b; else y3 |= b;
      }
      x0 = y0; x1 = y1; x2 = y2; x3 = y3;
    }
    // a byte -> its field: 0 -> 0, 1 -> 1, anything else -> 2
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t x = j < 4 ? x0 : j < 8 ? x1 : j < 12 ? x2 : x3;
      const uint32_t b = (x >> (8 * (j & 3))) & 0xFFu;
      w |= (b <= 1u ? b : 2u) << (2 * j);
    }
    return w;
  }
}

constexpr uint32_t AS_EVEN = 0x55555555u;   // bit 0 of each of the 16 fields

// the even bits of the fields lo .. hi - 1 of a group of 16 (0 <= lo < 16, lo < hi <= 16).  Shared by k_ancestry_score.hip and
// as_label_mask16.
__device__ __forceinline__ uint32_t as_range16(int lo, int hi) {
  const uint32_t below_hi = hi >= 16 ? 0xFFFFFFFFu : ((1u << (2 * hi)) - 1u);
  return below_hi & ~((1u << (2 * lo)) - 1u) & AS_EVEN;
}

// the even bits of those columns of [lo, hi) whose window carries label a in the row of labels lh; [lo, hi) lies inside the group of 16
// that starts at cg (an empty range gives 0).  A loop over the windows that meet the range: one turn unless a boundary falls inside,
// 16 turns at M = 1; the last window takes the remainder of the C columns.  A label is compared with a, never used as an index.  Shared
// by k_ancestry_pairs.hip and k_ancestry_ld.hip (k_ancestry_score.hip keeps a window running along its row instead).
__device__ __forceinline__ uint32_t as_label_mask16(const int32_t* lh, int32_t a, int64_t cg, int64_t lo, int64_t hi, int64_t C, int64_t M, int64_t W) {
  uint32_t m = 0;
  int64_t c = lo, k = lo / M;
  if (k > W - 1) k = W - 1;
  while (c < hi) {          // the columns [c, se) lie in window k
    const int64_t wend = (k == W - 1) ? C : (k + 1) * M;
    const int64_t se = hi < wend ? hi : wend;
    if (lh[k] == a) m |= as_range16((int)(c - cg), (int)(se - cg));
    c = se;
    ++k;
  }
  return m;
}

// of a group's fields f: the even bits of the observed calls (code 0 or 1), and of those of them that are ALT
__device__ __forceinline__ void as_obs_alt(uint32_t f, uint32_t* obs, uint32_t* alt) {
  *obs = ~(f >> 1) & AS_EVEN;
  *alt = f & *obs;
}

inline int64_t as_min_row_bytes(int row_kind, int64_t C) { return row_kind == GNX_ROWS_PACKED2 ? (C + 3) / 4 : C; }

inline int64_t as_win(int64_t c, int64_t M, int64_t W) { return std::min(c / M, W - 1); }
