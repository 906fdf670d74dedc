// gnx_rank.h — the rank quantisation shared by k_smooth_xgb_rk.hip and k_gnofix.hip (device code only).
//
// A tree of the smoother only ever asks "p < threshold" (xgboost: fvalue < split_condition -> left).  The model loader sorts the
// ensemble's distinct thresholds U[0..K) once (gnx_model_build.hip: build_xgb_rk); a base probability p is replaced by
// r(p) = #{k : U[k] <= p} (16 bits) and a node's threshold U[k] by k + 1, so that  p < U[k]  <=>  r(p) < k + 1: every walk takes
// the branch the float compare takes.  NaN -> 0xFFFF ("never less than a threshold").  The lookup table and its pieces, shared with
// the host: gnx_rank_table.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gnx_rank_table.h"
#include "gnx_window.h"  // gnx_slide_src

namespace {

// NV independent rank computations side by side: r = #{U[k] <= p}; NaN -> 0xFFFF ("never less than a threshold").
// One 16-byte gather from the model's table (gnx_rank_table.h) is the rank of nearly every probability; the bisection behind it
// runs only while some lane of the wave still has an open range (steps = 0 for a table whose buckets all fit their entry).
template <int NV>
__device__ __forceinline__ void ranks(const float* __restrict__ U, const GnxRankEntry* __restrict__ lut, int K, int bits, int steps,
                                      const float* p, uint32_t* r) {
#ifdef GNX_RANK_ABLATE
  // development only (scripts/dev/rank_ablate.sh): one conversion instead of the lookup — WRONG ranks, the same loads and stores;
  // what the kernel saves is the ceiling of anything a better table can win
#pragma unroll
  for (int i = 0; i < NV; ++i) r[i] = (uint32_t)(uint16_t)(int)(p[i] * (float)K);
#else
  int lo[NV], hi[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    typedef uint32_t rank_u32x4 __attribute__((ext_vector_type(4)));
    const rank_u32x4 e = reinterpret_cast<const rank_u32x4*>(lut)[gnx_rank_bucket(p[i], bits)];
    gnx_rank_head(e.x, __uint_as_float(e.y), __uint_as_float(e.z), __uint_as_float(e.w), p[i], lo[i], hi[i]);
  }
  for (int s = 0; s < steps; ++s) {
    bool open = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) open |= lo[i] < hi[i];
    if (!__any(open)) break;  // wave-uniform
    float u[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) u[i] = U[min((lo[i] + hi[i]) >> 1, K - 1)];
#pragma unroll
    for (int i = 0; i < NV; ++i) gnx_rank_step(u[i], p[i], lo[i], hi[i]);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) r[i] = (p[i] != p[i]) ? 0xFFFFu : (uint32_t)lo[i];
#endif
}

}  // namespace
