// k_smooth_xgb_h32.hip — the sliding-window tree smoother with LANE = HAPLOTYPE, 32 haplotypes per half-wave (GNX_SMOOTH_IMPL=h32).
//
// Same contract and the same arithmetic as k_smooth_xgb_rk.hip (slide_window + XGBClassifier.predict_proba + argmax, reference
// src/Smooth/utils.py:4-29, src/Smooth/smooth.py:40-65, src/Smooth/models.py:8-24; 16-bit ranks instead of float compares, leaves
// summed in tree order from base_score: margins, probabilities and labels bit-identical to the rank kernel).  What changes is who
// shares an LDS bank.
//
// k_smooth_xgb_rk puts 64 consecutive WINDOWS of one haplotype on a wave, so lanes that took different branches gather their ranks
// from unrelated addresses (a fifth of its LDS cycles are bank conflicts).  k_smooth_xgb_h64 (removed; sources at commit 8235b46) put 64
// HAPLOTYPES on a wave: conflict-free, but its 109 KB strip left one 16-wave block per CU and the two pipes no longer overlapped.
// `ds_read_u16` is banked per group of 32 lanes, so 32 haplotypes are enough: here lanes 0-31 and lanes 32-63 are the SAME 32
// haplotypes at two neighbouring windows, and a dword of the strip holds two neighbouring strip slots of one haplotype:
//   strip[slot pair q][class a][haplotype h] = rank(slot 2q) | rank(slot 2q + 1) << 16,   128 bytes per (q, a) row.
// Lane h of either half-wave reads bank h whatever node it sits on.  A block is 16 waves x 2 half-waves x 3 windows per lane = 96
// windows of 32 haplotypes; its strip (96 + S - 1 slots) is 76 KB at chr22 / A = 7: two blocks = 32 waves per CU.
//
// The slot of a feature is the window's own strip position plus the feature's window offset, and its parity picks the half of the
// dword.  The low half-wave takes the block's even positions and the high half-wave the odd ones, and the model loader lays every
// tree's nodes out twice (gnx_model_build.hip, SmoothXGBDev::h3_packed): once with the byte offsets of slot s, once with those of
// slot s + 1 counted from the even position before the window.  Both halves of a wave then share one strip origin per window
// pair and the rank address stays ONE add (origin + the node's 16-bit offset).  The walk is the pointer-node walk of
// k_smooth_xgb_rk<.., PTR>: 3 VALU and 2 LDS reads per level, two trees side by side, levels 0 and 1 from the tree's first 16 bytes.
#include <cstdio>
#include <cstdlib>

#include "gnx_internal.h"
#include "gnx_exp.h"
#include "gnx_rank.h"

namespace {

constexpr int HB = 32;                     // haplotypes per block = lanes of a half-wave
constexpr int RW = 3;                      // windows per lane
constexpr int NWAVE = 16;
constexpr int WPW = 2 * RW;                // windows per wave: positions 6 wave + 2 k + half
constexpr int WPB = NWAVE * WPW;
constexpr int THREADS = NWAVE * 64;
constexpr int TB = GNX_H32_TREE_BYTES;
static_assert(WPB == GNX_H32_WPB, "the model loader sizes the staging groups for this block");

#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(3))) T* lds_at(uint32_t a) {
  return (const __attribute__((address_space(3))) T*)(uintptr_t)a;
}
#else
template <typename T>
__device__ const T* lds_at(uint32_t) { return nullptr; }  // host pass: never called
#endif
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t step_ptr(uint32_t w0, uint32_t w1, uint32_t r) {
  uint32_t p;
  asm("v_cmp_le_u32_sdwa vcc, %[n], %[r] src0_sel:WORD_1 src1_sel:DWORD\n\t"
      "v_cndmask_b32_sdwa %[p], %[w], %[w], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1"
      : [p] "=v"(p)
      : [n] "v"(w0), [r] "v"(r), [w] "v"(w1)
      : "vcc");
  return p;
}
// level 0: the level-1 node {w0, w1} is one of two candidates from the tree top, picked by the root's compare
__device__ __forceinline__ void first_ptr(uint32_t root, uint32_t r, uint32_t l0, uint32_t r0, uint32_t l1, uint32_t r1, uint32_t& w0,
                                          uint32_t& w1) {
  asm("v_cmp_le_u32_sdwa vcc, %[n], %[r] src0_sel:WORD_1 src1_sel:DWORD\n\t"
      "v_cndmask_b32 %[x], %[l0], %[r0], vcc\n\t"
      "v_cndmask_b32 %[y], %[l1], %[r1], vcc"
      : [x] "=&v"(w0), [y] "=&v"(w1)
      : [n] "v"(root), [r] "v"(r), [l0] "v"(l0), [r0] "v"(r0), [l1] "v"(l1), [r1] "v"(r1)
      : "vcc");
}

// NT trees (tb, tb + TB, ...: LDS addresses of the lane's copy of the node slots) side by side for the RW windows of a lane.
// rb[k] = LDS address of the lane's dword in the row (slot pair of window k, class 0).
template <int NT>
__device__ __forceinline__ void walk_h32(uint32_t tb, const uint32_t* rb, float* psum) {
  constexpr int NC = NT * RW;
  uint32_t w0[NC], w1[NC], r[NC], p[NC];
  u32x4 top[NT];  // {w0 of node 2, w0 of node 3, w0 of the root, w1 of node 2}
#pragma unroll
  for (int t = 0; t < NT; ++t) top[t] = *lds_at<u32x4>(tb + t * TB);
  constexpr uint32_t SIB = 16u * 0x10001u;  // node 3's children sit right behind node 2's
#pragma unroll
  for (int c = 0; c < NC; ++c) r[c] = *lds_at<uint16_t>(rb[c % RW] + (top[c / RW].z & 0xffffu));
#pragma unroll
  for (int c = 0; c < NC; ++c)
    first_ptr(top[c / RW].z, r[c], top[c / RW].x, top[c / RW].y, top[c / RW].w, top[c / RW].w + SIB, w0[c], w1[c]);
#pragma unroll
  for (int c = 0; c < NC; ++c) r[c] = *lds_at<uint16_t>(rb[c % RW] + (w0[c] & 0xffffu));
#pragma unroll
  for (int c = 0; c < NC; ++c) p[c] = step_ptr(w0[c], w1[c], r[c]);
#pragma unroll
  for (int d = 2; d < 4; ++d) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const u32x2 nd = *lds_at<u32x2>(p[c]);
      w0[c] = nd.x;
      w1[c] = nd.y;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = *lds_at<uint16_t>(rb[c % RW] + (w0[c] & 0xffffu));
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = step_ptr(w0[c], w1[c], r[c]);
  }
  float lf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) lf[c] = *lds_at<float>(p[c]);
#pragma unroll
  for (int t = 0; t < NT; ++t)  // tree order
#pragma unroll
    for (int k = 0; k < RW; ++k) psum[k] += lf[t * RW + k];
}

// gw = waves whose probabilities the LDS holds at once in the output transpose (a power of two, the launcher's choice)
// IMG: the strip is copied from the rank image the base pass wrote (SmoothXGBLaunch::rk16) instead of ranked from B
template <bool IMG>
__global__ __launch_bounds__(THREADS, 8) void k_smooth_xgb_h32(SmoothXGBLaunch L, int gw) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int A = L.A, W = L.W, S = L.S, pad = (S + 1) / 2;
  const int buf_bytes = L.d.h3_max_group * TB;   // multiple of 16, at most 5 KB
  const int P = WPB + S - 1;                      // strip slots held
  uint8_t* tbuf0 = lds;                           // the trees first: node addresses must fit 16 bits
  uint8_t* tbuf1 = tbuf0 + buf_bytes;
  uint8_t* strip = tbuf1 + buf_bytes;             // [(P + 1) / 2][A][32] dwords
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane & 31, hv = lane >> 5;
  const int64_t hb = blockIdx.y, h0 = hb * HB;
  const int w0 = blockIdx.x * WPB;

  // ---- stage the reflected base-probability strip as ranks ---------------------------------------------------------------
  // a wave takes 16 haplotypes x 4 consecutive (slot, class) elements at a time: 16-byte runs of B on the way in, and on the way
  // out the 8 haplotypes of a half-wave spread over 8 banks (4 rows each: the transposition's conflicts, 4-way instead of 32-way).
  // A thread keeps its haplotype; its elements are 32 apart, so (slot, class) advance by a fixed step: no division per element
  // Only a haplotype's first and last window block touch the reflection; a block whose slots all lie inside the chromosome reads
  // its strip as ONE run of P * A elements per haplotype (element rr of the strip is element rr of the run): no slide_src, no
  // clamps of the slot, no index arithmetic per element.  blockIdx.x decides, so the branch is uniform.
  if constexpr (IMG) {
    // The image holds the ranks already, one 64-byte row of the block's 32 haplotypes per (window, class): row (q, a) of the strip
    // is the rows of its two source windows interleaved.  Four threads per strip row, 8 haplotypes each: two 16-byte loads, two
    // 16-byte LDS writes (64 lanes = 2 KB in a run: no conflicts).  The source windows are uniform over a row, so the reflection
    // costs nothing per element; a thread's rows are THREADS / 4 apart, so (q, a) advance by a fixed step.
    constexpr int RPI = THREADS / 4;                // strip rows per iteration of the block
    const int n_rows = ((P + 1) / 2) * A;
    const uint16_t* img = L.rk16 + (size_t)hb * W * A * HB + (tid & 3) * 8;
    const int dq = RPI / A, da = RPI - dq * A;
    int row = tid >> 2;
    int q = row / A, a = row - q * A;
    for (int it = 0; it < (n_rows + RPI - 1) / RPI; ++it, row += RPI) {
      const bool ok = row < n_rows;
      const int qc = ok ? q : 0, ac = ok ? a : 0;  // clamped: loads stay unconditional
      const int s0 = gnx_slide_src(min(w0 + 2 * qc, W + 2 * pad - 1), W, pad);
      const int s1 = gnx_slide_src(min(w0 + 2 * qc + 1, W + 2 * pad - 1), W, pad);
      const u32x4 x = *reinterpret_cast<const u32x4*>(img + ((size_t)s0 * A + ac) * HB);
      const u32x4 y = *reinterpret_cast<const u32x4*>(img + ((size_t)s1 * A + ac) * HB);
      u32x4 lo4, hi4;  // haplotypes 0-3 and 4-7 of the thread's eight: rank(2q) | rank(2q + 1) << 16
      lo4.x = (x.x & 0xffffu) | (y.x << 16);
      lo4.y = (x.x >> 16) | (y.x & 0xffff0000u);
      lo4.z = (x.y & 0xffffu) | (y.y << 16);
      lo4.w = (x.y >> 16) | (y.y & 0xffff0000u);
      hi4.x = (x.z & 0xffffu) | (y.z << 16);
      hi4.y = (x.z >> 16) | (y.z & 0xffff0000u);
      hi4.z = (x.w & 0xffffu) | (y.w << 16);
      hi4.w = (x.w >> 16) | (y.w & 0xffff0000u);
      if (ok) {
        u32x4* dst = reinterpret_cast<u32x4*>(strip + (size_t)row * 128 + (tid & 3) * 32);
        dst[0] = lo4;
        dst[1] = hi4;
      }
      a += da;
      q += dq;
      if (a >= A) { a -= A; ++q; }
    }
  } else {
    constexpr int NV = 4;
    const int per_h = P * A;
    const int hl = (wave & 1) * 16 + (lane >> 2);
    const size_t row = (size_t)min(h0 + hl, L.N - 1) * W;
    const int dq = 32 / A, da = 32 - dq * A;
    int rr = (wave >> 1) * 4 + (lane & 3);
    int q = rr / A, a = rr - q * A;
    const bool interior = w0 >= pad && w0 + P <= pad + W;
    const size_t run0 = (row + (size_t)(interior ? w0 - pad : 0)) * A;
    for (; rr < per_h; rr += NV * 32) {
      float p[NV];
      uint32_t r[NV];
      int dst[NV];
      bool ok[NV];
      if (interior) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          ok[i] = rr + i * 32 < per_h;
          const size_t idx = run0 + (size_t)min(rr + i * 32, per_h - 1);  // clamped: loads stay unconditional
          p[i] = L.b_is_f64 ? (float)reinterpret_cast<const double*>(L.B)[idx] : reinterpret_cast<const float*>(L.B)[idx];
          dst[i] = ((q >> 1) * A + a) * 128 + hl * 4 + (q & 1) * 2;  // never stored when !ok
          a += da;
          q += dq;
          if (a >= A) { a -= A; ++q; }
        }
      } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          ok[i] = rr + i * 32 < per_h;
          const int qc = ok[i] ? q : P - 1, ac = ok[i] ? a : A - 1;  // clamped: loads stay unconditional
          const int j = min(w0 + qc, W + 2 * pad - 1);
          const size_t idx = (row + gnx_slide_src(j, W, pad)) * A + ac;
          p[i] = L.b_is_f64 ? (float)reinterpret_cast<const double*>(L.B)[idx] : reinterpret_cast<const float*>(L.B)[idx];
          dst[i] = ((qc >> 1) * A + ac) * 128 + hl * 4 + (qc & 1) * 2;
          a += da;
          q += dq;
          if (a >= A) { a -= A; ++q; }
        }
      }
      ranks<NV>(L.d.rk_thr, L.d.rk_lut, L.d.rk_K, L.d.rk_bits, L.d.rk_steps, p, r);
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (ok[i]) *reinterpret_cast<uint16_t*>(strip + dst[i]) = (uint16_t)r[i];
    }
  }

  const int64_t n = h0 + h;
  uint32_t rb[RW];
  bool valid[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    rb[k] = (uint32_t)(uintptr_t)strip + (uint32_t)(((wave * RW + k) * A) * 128 + h * 4);
    valid[k] = (n < L.N) && (w0 + wave * WPW + 2 * k + hv < W);
  }
  // margins parked class-major, [class][haplotype block][window][32 lanes]: whole 128-byte lines
  const size_t cls_stride = (size_t)gridDim.y * W * HB;
  float* mrow = L.marg + ((size_t)hb * W + w0 + wave * WPW + hv) * HB + h;

  // ---- tree groups through the double-buffered LDS window ----
  const int ng = L.d.h3_n_groups;
  uint4 stg;
  // unconditional clamped loads: no branch around a load
#define GNX_G_LOAD(g)                                                                               \
  {                                                                                                 \
    const int t0_ = L.d.h3_group_tree0[g], t1_ = L.d.h3_group_tree0[(g) + 1];                       \
    const int last_ = (t1_ - t0_) * TB / 16 - 1;                                                    \
    stg = reinterpret_cast<const uint4*>(L.d.h3_packed + (size_t)t0_ * TB)[min(tid, last_)];        \
  }
#define GNX_G_STORE(dst)                                                                            \
  {                                                                                                 \
    /* child addresses: relative to the group -> LDS addresses; pieces 0-7 and 12-19 of a tree are node slots */ \
    const int pc_ = (tid * 16 % TB) >> 4;                                                           \
    const bool node_ = pc_ < 8 || pc_ >= 12;                                                        \
    const uint32_t add_ = node_ ? (uint32_t)(uintptr_t)(dst) * 0x10001u : 0u;                       \
    stg.w += add_;                                                                                  \
    stg.y += (pc_ == 0 || pc_ == 12) ? 0u : add_;                                                   \
    if (tid * 16 < buf_bytes) *reinterpret_cast<uint4*>((dst) + (size_t)tid * 16) = stg;            \
  }
  float psum[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) psum[k] = 0.f;

  GNX_G_LOAD(0);
  GNX_G_STORE(tbuf0);
  __syncthreads();

  int cur_class = L.d.h3_group_class[0];
  for (int g = 0; g < ng; ++g) {
    uint8_t* cur = (g & 1) ? tbuf1 : tbuf0;
    uint8_t* nxt = (g & 1) ? tbuf0 : tbuf1;
    const int gn = min(g + 1, ng - 1);  // clamped: the last iteration re-fetches its own group
    GNX_G_LOAD(gn);
    const int cls = L.d.h3_group_class[g];
    if (cls != cur_class) {
#pragma unroll
      for (int k = 0; k < RW; ++k) {
        if (valid[k]) mrow[(size_t)cur_class * cls_stride + (size_t)(2 * k) * HB] = L.d.base_score + psum[k];
        psum[k] = 0.f;
      }
      cur_class = cls;
    }
    const int nt = L.d.h3_group_tree0[g + 1] - L.d.h3_group_tree0[g];
    const uint32_t tb = (uint32_t)(uintptr_t)cur + (uint32_t)hv * 192u;  // the half-wave's copy of the node slots
    int t = 0;
    for (; t + 2 <= nt; t += 2) walk_h32<2>(tb + (uint32_t)t * TB, rb, psum);
    for (; t < nt; ++t) walk_h32<1>(tb + (uint32_t)t * TB, rb, psum);
    GNX_G_STORE(nxt);
    __syncthreads();
  }
#undef GNX_G_LOAD
#undef GNX_G_STORE
#pragma unroll
  for (int k = 0; k < RW; ++k)
    if (valid[k]) mrow[(size_t)cur_class * cls_stride + (size_t)(2 * k) * HB] = L.d.base_score + psum[k];

  // ---- softmax (xgboost common/math.h Softmax) + argmax ----
  // Lanes are haplotypes, W * A floats apart in the outputs, so the probabilities go through the LDS (the strip is dead after
  // the loop's last barrier): gw waves at a time park theirs in a tile [32 haplotypes][6 gw windows x A] with an odd row pitch,
  // and the block writes every haplotype's 6 gw * A consecutive floats (and its 6 gw labels) as one run.
  float* tile = reinterpret_cast<float*>(lds);
  const int rowlen = gw * WPW * A, pitch = rowlen | 1;
  for (int g0 = 0; g0 < NWAVE; g0 += gw) {
    if (wave >= g0 && wave < g0 + gw) {
#pragma unroll
      for (int k = 0; k < RW; ++k) {
        if (!valid[k]) continue;
        const float* mg = mrow + (size_t)(2 * k) * HB;
        float* o = tile + (size_t)h * pitch + ((wave - g0) * WPW + 2 * k + hv) * A;
        float wmax = mg[0];
        for (int a = 1; a < A; ++a) wmax = fmaxf(mg[(size_t)a * cls_stride], wmax);
        double wsum = 0.0;
        for (int a = 0; a < A; ++a) {
          const float e = gnx_softmax_exp(mg[(size_t)a * cls_stride] - wmax);
          o[a] = e;
          wsum += (double)e;
        }
        const float fs = (float)wsum;
        for (int a = 0; a < A; ++a) o[a] = o[a] / fs;
      }
    }
    __syncthreads();
    const int wb = w0 + g0 * WPW;
    for (int e = tid; e < HB * rowlen; e += THREADS) {
      const int hl = e / rowlen, c = e - hl * rowlen;
      const int64_t nn = h0 + hl;
      if (nn < L.N && wb + c / A < W) {
        const float p = tile[(size_t)hl * pitch + c];
        const size_t idx = ((size_t)nn * W + wb) * A + c;
        L.proba[idx] = p;
        if (L.proba64) L.proba64[idx] = (double)p;
      }
    }
    if (L.labels) {
      const int nwl = gw * WPW;
      for (int e = tid; e < HB * nwl; e += THREADS) {
        const int hl = e / nwl, wl = e - hl * nwl;
        const int64_t nn = h0 + hl;
        if (nn < L.N && wb + wl < W) {
          const float* o = tile + (size_t)hl * pitch + wl * A;
          int best = 0;
          float bv = -1.f;
          for (int a = 0; a < A; ++a) {
            const float p = o[a];
            if (p > bv) { bv = p; best = a; }
          }
          L.labels[(size_t)nn * W + wb + wl] = best;
        }
      }
    }
    __syncthreads();
  }
}

size_t lds_need(const SmoothXGBDev& d, int A, int S) { return gnx_h32_lds_bytes(A, S, d.h3_max_group); }

}  // namespace

bool gnx_smooth_h32_fits(const SmoothXGBDev& d, int A, int S) {
  // two blocks per CU (32 waves) or nothing: with one block the walk's two pipes stop overlapping (k_smooth_xgb_h64)
  return d.h3_packed && d.rk_thr && d.D == 4 && lds_need(d, A, S) <= (size_t)80 * 1024;
}

hipError_t gnx_launch_smooth_xgb_h32(const SmoothXGBLaunch& L, hipStream_t s) {
  if (L.N <= 0) return hipSuccess;
  if (!gnx_smooth_h32_fits(L.d, L.A, L.S)) return hipErrorInvalidValue;  // declined: the caller takes k_smooth_xgb_rk
  const size_t lds = lds_need(L.d, L.A, L.S);
  int gw = NWAVE;  // the output tile of gw waves must fit what the walk had
  while (gw > 1 && (size_t)HB * ((size_t)(gw * WPW * L.A) | 1) * 4 > lds) gw >>= 1;
  if ((size_t)HB * ((size_t)(gw * WPW * L.A) | 1) * 4 > lds) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((L.W + WPB - 1) / WPB), (unsigned)((L.N + HB - 1) / HB));
  if (L.rk16) {
    GNX_LDS_OPTIN(lds, k_smooth_xgb_h32<true>);
    hipLaunchKernelGGL(k_smooth_xgb_h32<true>, grid, dim3(THREADS), lds, s, L, gw);
  } else {
    GNX_LDS_OPTIN(lds, k_smooth_xgb_h32<false>);
    hipLaunchKernelGGL(k_smooth_xgb_h32<false>, grid, dim3(THREADS), lds, s, L, gw);
  }
  return hipGetLastError();
}
