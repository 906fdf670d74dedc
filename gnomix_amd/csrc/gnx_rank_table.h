// gnx_rank_table.h — the table behind the rank quantisation (gnx_rank.h), plain C++: the loader builds it on the host
// (gnx_model_build.hip: build_xgb_rk), the kernels look a probability up with the pieces below, and tests/test_rank_table_host.py
// compiles the same pieces into a stand-alone program and checks them against brute force.
//
// U[0..K) = the ensemble's sorted distinct finite thresholds, r(p) = #{k : U[k] <= p}.  The table has NB = 2^bits buckets keyed on
// p * NB (a power of two: the product is exact, so bucket b holds exactly the p with b / NB <= p < (b + 1) / NB; bucket 0 also
// everything below and NaN, the last bucket everything above).  An entry is 16 bytes, ONE gather:
//   lohi = lo | hi << 16   with lo = #{U < lower edge}, hi = #{U < upper edge}: r(p) lies in [lo, hi]
//   t[i] = U[lo + i] for i < min(3, hi - lo), NaN behind them (NaN <= p never holds)
// so r(p) = lo + (t0 <= p) + (t1 <= p) + (t2 <= p) wherever the bucket holds at most three thresholds, or p lies below its third:
// no search and no second gather.  Only a p at or above the third threshold of a fuller bucket searches U[lo + 3 .. hi), by
// bisection as before; `steps` = the smallest number of bisections that resolves the fullest bucket's remainder (0 when no bucket
// holds more than three).  The bucket count is chosen per model (gnx_rank_table_build).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GNX_RANK_HD __host__ __device__ __forceinline__
#else
#define GNX_RANK_HD inline
#endif

constexpr int GNX_RANK_INLINE = 3;     // thresholds carried by an entry
constexpr int GNX_RANK_MIN_BITS = 10;  // 16 KB: stays in a CU's L1
constexpr int GNX_RANK_MAX_BITS = 16;  // 1 MB: L2

struct GnxRankEntry {
  uint32_t lohi;
  float t[GNX_RANK_INLINE];
};
static_assert(sizeof(GnxRankEntry) == 16, "one 16-byte gather per probability");

GNX_RANK_HD int gnx_rank_bucket(float p, int bits) {
  const float nb = (float)(1 << bits);
  const float sc = p * nb;
  // NaN -> 0 (the max drops it); the caller overrides a NaN's rank
  return (int)__builtin_fminf(__builtin_fmaxf(sc, 0.0f), nb - 1.0f);
}

// the entry's part of the rank: [lo, hi] = what is left to search (lo == hi: lo is the rank)
GNX_RANK_HD void gnx_rank_head(uint32_t lohi, float t0, float t1, float t2, float p, int& lo, int& hi) {
  const int l = (int)(lohi & 0xffffu), h = (int)(lohi >> 16);
  const int c = l + (t0 <= p ? 1 : 0) + (t1 <= p ? 1 : 0) + (t2 <= p ? 1 : 0);
  lo = c;
  hi = (t2 <= p) ? h : c;  // all three at or below p: c = l + 3 <= h and the rest of the bucket is open
}

// one bisection of [lo, hi] against u = U[min((lo + hi) >> 1, K - 1)]; a closed range stays as it is
GNX_RANK_HD void gnx_rank_step(float u, float p, int& lo, int& hi) {
  const int mid = (lo + hi) >> 1;
  const bool open = lo < hi;
  const bool up = open && (u <= p);
  hi = (open && !up) ? mid : hi;
  lo = up ? mid + 1 : lo;
}

// ---- host side: the builder and a scalar restatement of the lookup ----
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

struct GnxRankTable {
  std::vector<GnxRankEntry> lut;
  int bits = 0, steps = 0, fullest = 0;
};

// entries and the bisection count of a table of 2^bits buckets over the sorted distinct finite thresholds U (at least one)
inline void gnx_rank_table_fill(const std::vector<float>& U, int bits, GnxRankTable& T) {
  const int K = (int)U.size(), NB = 1 << bits;
  T.bits = bits;
  T.steps = 0;
  T.fullest = 0;
  T.lut.assign((size_t)NB, GnxRankEntry());
  for (int b = 0; b < NB; ++b) {
    // b / NB is exact in float for NB <= 2^16
    const int lo = b == 0 ? 0 : (int)(std::lower_bound(U.begin(), U.end(), (float)b / (float)NB) - U.begin());
    const int hi = b == NB - 1 ? K : (int)(std::lower_bound(U.begin(), U.end(), (float)(b + 1) / (float)NB) - U.begin());
    GnxRankEntry& e = T.lut[(size_t)b];
    e.lohi = (uint32_t)lo | ((uint32_t)hi << 16);
    for (int i = 0; i < GNX_RANK_INLINE; ++i) e.t[i] = i < hi - lo ? U[(size_t)(lo + i)] : std::numeric_limits<float>::quiet_NaN();
    const int rest = hi - lo - GNX_RANK_INLINE;  // what a search has to tell apart: rest + 1 ranks
    int st = 0;
    while (rest > 0 && (1 << st) < rest + 1) ++st;
    T.steps = std::max(T.steps, st);
    T.fullest = std::max(T.fullest, hi - lo);
  }
}

// The sizing rule: the smallest table, from 2^10 buckets up, whose fullest bucket holds at most three thresholds —
// every rank is then the one gather — and 2^max_bits when none does.  force_bits > 0 (GNX_RK_BITS, development) overrides it.
inline void gnx_rank_table_build(const std::vector<float>& U, int force_bits, GnxRankTable& T, int max_bits = GNX_RANK_MAX_BITS) {
  if (force_bits > 0) {
    gnx_rank_table_fill(U, std::max(1, std::min(GNX_RANK_MAX_BITS, force_bits)), T);
    return;
  }
  for (int bits = GNX_RANK_MIN_BITS;; ++bits) {
    gnx_rank_table_fill(U, bits, T);
    if (T.steps == 0 || bits >= max_bits) return;
  }
}

// the kernels' lookup, one probability at a time (host restatement of gnx_rank.h: ranks<NV>)
inline uint32_t gnx_rank_lookup(const std::vector<float>& U, const GnxRankTable& T, float p) {
  const GnxRankEntry& e = T.lut[(size_t)gnx_rank_bucket(p, T.bits)];
  int lo, hi;
  gnx_rank_head(e.lohi, e.t[0], e.t[1], e.t[2], p, lo, hi);
  const int K = (int)U.size();
  for (int s = 0; s < T.steps; ++s) gnx_rank_step(U[(size_t)std::min((lo + hi) >> 1, K - 1)], p, lo, hi);
  return (p != p) ? 0xFFFFu : (uint32_t)lo;
}
