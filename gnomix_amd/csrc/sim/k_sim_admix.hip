// k_sim_admix.hip — the admixture simulator's data: the N x C training matrix, its per-SNP ancestry and its window labels,
// built from segment tables drawn on the host (gnomix_amd/simulate.py).
//
// Reference: admix() (src/laidataset.py:119-176) copies founder slices into each simulated haplotype, segment by segment, in a
// Python loop; write_output (laidataset.py:180-201) stacks them into mat_vcf_2d.npy / mat_map.npy; window_reshape
// (src/preprocess.py:37-59) reduces the ancestry rows to one label per window with scipy.stats.mode.  The random draws stay on
// the host (they must follow numpy's stream exactly); what they produce is a few (begin, source) pairs per haplotype.
//
// k_sim_admix: block (tile, n) owns 4096 columns of haplotype n, 16 per lane.  A lane finds the segment covering its first
// column by a binary search in that haplotype's list (a handful of entries, cached).  A chunk inside one segment is one 16-byte
// load of the founder row and one 16-byte store to X (and a splat of the ancestry byte to the ancestry row); a chunk that a
// boundary or the end of the row cuts is assembled byte by byte in four registers.  Lane g of the grid also labels window g of
// the row from the segments' overlaps with it (no bytes re-read).  Loads and stores use the widest access their address
// allows (rows whose stride is not a multiple of 16 are still correct, only narrower).
//
// k_sim_check_tables / k_sim_check_founders: validation before anything is written; the first offence is kept with atomicMin.
#include "../gnx_internal.h"

namespace {

constexpr int SIM_THREADS = 256;
constexpr int SIM_CHUNK = 16;
constexpr int64_t SIM_TILE = (int64_t)SIM_THREADS * SIM_CHUNK;
constexpr unsigned SIM_MAX_GRID_Y = 65535;

struct SimArgs {
  const int8_t* F;
  int64_t nF, ldf, C, M, W;
  const int64_t* seg_off;
  const int32_t* seg_begin;
  const int32_t* seg_src;
  const uint8_t* anc_of_src;
  int32_t A;
  int64_t N;
  int8_t* X;
  int64_t ldx;
  int32_t* Y;
  uint8_t* anc;
};

__device__ __forceinline__ void load16(const int8_t* p, uint32_t w[4]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
    const uint4 v = *(const uint4*)p;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else if ((a & 7) == 0) {
    const uint2 v0 = ((const uint2*)p)[0], v1 = ((const uint2*)p)[1];
    w[0] = v0.x; w[1] = v0.y; w[2] = v1.x; w[3] = v1.y;
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = ((const uint32_t*)p)[k];
  } else {
    const uint8_t* b = (const uint8_t*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
  }
}

__device__ __forceinline__ void store16(void* p, const uint32_t w[4]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
    *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
  } else if ((a & 7) == 0) {
    ((uint2*)p)[0] = make_uint2(w[0], w[1]);
    ((uint2*)p)[1] = make_uint2(w[2], w[3]);
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) ((uint32_t*)p)[k] = w[k];
  } else {
    uint8_t* b = (uint8_t*)p;
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

// the segment of [s0, s1) that covers column c: the last one whose begin is <= c (begin[s0] == 0 <= c)
__device__ __forceinline__ int64_t find_seg(const int32_t* __restrict__ begin, int64_t s0, int64_t s1, int64_t c) {
  int64_t lo = s0, hi = s1 - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(SIM_THREADS) void k_sim_admix(SimArgs a) {
  const int64_t g = (int64_t)blockIdx.x * SIM_THREADS + threadIdx.x;
  const int64_t c0 = g * SIM_CHUNK;
  for (int64_t n = blockIdx.y; n < a.N; n += gridDim.y) {
    const int64_t s0 = a.seg_off[n], s1 = a.seg_off[n + 1];
    if (c0 < a.C) {
      int64_t s = find_seg(a.seg_begin, s0, s1, c0);
      int64_t e = s + 1 < s1 ? a.seg_begin[s + 1] : a.C;
      int32_t src = a.seg_src[s];
      const int64_t cnt = a.C - c0 < SIM_CHUNK ? a.C - c0 : SIM_CHUNK;
      int8_t* xr = a.X + n * a.ldx + c0;
      uint8_t* ar = a.anc ? a.anc + n * a.C + c0 : nullptr;
      uint32_t w[4], an[4];
      if (cnt == SIM_CHUNK && c0 + SIM_CHUNK <= e) {
        load16(a.F + (int64_t)src * a.ldf + c0, w);
        store16(xr, w);
        if (ar) {
          const uint32_t splat = 0x01010101u * a.anc_of_src[src];
          an[0] = an[1] = an[2] = an[3] = splat;
          store16(ar, an);
        }
      } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
        an[0] = an[1] = an[2] = an[3] = 0u;
#pragma unroll
        for (int j = 0; j < SIM_CHUNK; ++j) {
          if (j < cnt) {
            const int64_t c = c0 + j;
            while (c >= e) {
              ++s;
              src = a.seg_src[s];
              e = s + 1 < s1 ? a.seg_begin[s + 1] : a.C;
            }
            w[j >> 2] |= (uint32_t)(uint8_t)a.F[(int64_t)src * a.ldf + c] << (8 * (j & 3));
            an[j >> 2] |= (uint32_t)a.anc_of_src[src] << (8 * (j & 3));
          }
        }
        if (cnt == SIM_CHUNK) {
          store16(xr, w);
          if (ar) store16(ar, an);
        } else {
#pragma unroll
          for (int j = 0; j < SIM_CHUNK; ++j) {
            if (j < cnt) {
              xr[j] = (int8_t)(w[j >> 2] >> (8 * (j & 3)));
              if (ar) ar[j] = (uint8_t)(an[j >> 2] >> (8 * (j & 3)));
            }
          }
        }
      }
    }
    if (g < a.W) {
      // window_reshape: windows 0..W-2 are [w M, (w+1) M), the last one [(W-1) M, C); label = the most frequent ancestry,
      // ties to the smallest code (scipy.stats.mode).  Counts are segment overlaps: for each ancestry met in the window, the
      // overlaps of all segments of that ancestry (a window meets few segments; no per-class array, no scratch).
      const int64_t lo = g * a.M, hi = g == a.W - 1 ? a.C : lo + a.M;
      const int64_t s_lo = find_seg(a.seg_begin, s0, s1, lo);
      int best = 0;
      int64_t best_n = -1;
      for (int64_t t = s_lo; t < s1 && a.seg_begin[t] < hi; ++t) {
        const int at = a.anc_of_src[a.seg_src[t]];
        int64_t n_at = 0;
        for (int64_t u = s_lo; u < s1 && a.seg_begin[u] < hi; ++u) {
          if (a.anc_of_src[a.seg_src[u]] != at) continue;
          const int64_t b = a.seg_begin[u] > lo ? a.seg_begin[u] : lo;
          const int64_t e = u + 1 < s1 && a.seg_begin[u + 1] < hi ? a.seg_begin[u + 1] : hi;
          n_at += e - b;
        }
        if (n_at > best_n || (n_at == best_n && at < best)) {
          best = at;
          best_n = n_at;
        }
      }
      a.Y[n * a.W + g] = best;
    }
  }
}

// err[0] = min over invalid haplotypes of (n << 3 | reason): 1 no segment, 2 first begin != 0, 3 begins not increasing or >= C,
// 4 source out of range, 5 source is not a founder (its ancestry code >= A)
__global__ __launch_bounds__(SIM_THREADS) void k_sim_check_tables(const int64_t* __restrict__ seg_off, const int32_t* __restrict__ begin,
                                                                  const int32_t* __restrict__ srcs, const uint8_t* __restrict__ anc_of_src,
                                                                  int64_t nF, int32_t A, int64_t C, int64_t N, unsigned long long* err) {
  const int64_t n = (int64_t)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (n >= N) return;
  const int64_t s0 = seg_off[n], s1 = seg_off[n + 1];
  int reason = 0;
  if (s1 <= s0) reason = 1;
  else if (begin[s0] != 0) reason = 2;
  for (int64_t s = s0; s < s1 && !reason; ++s) {
    if (begin[s] >= C || (s > s0 && begin[s] <= begin[s - 1])) reason = 3;
    else if (srcs[s] < 0 || srcs[s] >= nF) reason = 4;
    else if (anc_of_src[srcs[s]] >= A) reason = 5;
  }
  if (reason) atomicMin(&err[0], ((unsigned long long)n << 3) | (unsigned long long)reason);
}

// err[1] = min over founder rows (anc_of_src[r] < A) of r * C + c where F[r, c] is neither 0 nor 1
__global__ __launch_bounds__(SIM_THREADS) void k_sim_check_founders(const int8_t* __restrict__ F, int64_t nF, int64_t ldf, int64_t C,
                                                                    const uint8_t* __restrict__ anc_of_src, int32_t A, unsigned long long* err) {
  const int64_t c0 = ((int64_t)blockIdx.x * SIM_THREADS + threadIdx.x) * SIM_CHUNK;
  if (c0 >= C) return;
  for (int64_t r = blockIdx.y; r < nF; r += gridDim.y) {
    if (anc_of_src[r] >= A) continue;
    const int8_t* p = F + r * ldf + c0;
    const int64_t cnt = C - c0 < SIM_CHUNK ? C - c0 : SIM_CHUNK;
    int64_t bad = -1;
    if (cnt == SIM_CHUNK) {
      uint32_t w[4];
      load16(p, w);
      if ((w[0] | w[1] | w[2] | w[3]) & 0xFEFEFEFEu) {
#pragma unroll
        for (int j = SIM_CHUNK - 1; j >= 0; --j)
          if ((w[j >> 2] >> (8 * (j & 3))) & 0xFEu) bad = j;
      }
    } else {
      for (int64_t j = cnt - 1; j >= 0; --j)
        if ((uint8_t)p[j] & 0xFEu) bad = j;
    }
    if (bad >= 0) atomicMin(&err[1], (unsigned long long)(r * C + c0 + bad));
  }
}

}  // namespace

extern "C" int gnx_simulate_admix_dev(gnx_ctx* ctx, const int8_t* dF, int64_t n_founder_haps, int64_t ldf, int64_t C, int64_t M,
                                      const int64_t* d_seg_off, const int32_t* d_seg_begin, const int32_t* d_seg_src,
                                      const uint8_t* d_anc_of_src, int32_t A, int64_t N, int8_t* dX, int64_t ldx, int32_t* dY,
                                      uint8_t* d_anc) {
  if (!ctx) return GNX_EINVAL;
  if (N < 0 || C < 1 || C > INT32_MAX || M < 1 || M > C || n_founder_haps < 1 || ldf < C || ldx < C || A < 1 || A > GNX_SIM_MAX_A)
    return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: bad arguments (need N >= 0, 1 <= M <= C < 2^31, n_founder_haps >= 1, ldf >= C, "
                                     "ldx >= C, 1 <= A <= " + std::to_string(GNX_SIM_MAX_A) + ")");
  if (N == 0) return GNX_OK;
  if (!dF || !d_seg_off || !d_seg_begin || !d_seg_src || !d_anc_of_src || !dX || !dY)
    return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: NULL array");
  GNX_BIND_DEVICE(ctx);
  // the offsets first, on the host: every later device read of the tables stays inside [0, seg_off[N])
  std::vector<int64_t> off((size_t)N + 1);
  HIPCHK(ctx, hipMemcpyAsync(off.data(), d_seg_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (off[0] != 0) return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: seg_off[0] must be 0");
  for (int64_t n = 0; n < N; ++n)
    if (off[n + 1] <= off[n])
      return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: haplotype " + std::to_string(n) + " has no segment (seg_off must increase)");
  if (off[N] > INT32_MAX) return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: more than 2^31 - 1 segments");
  int rc = gnx_ws_reserve(ctx, ctx->ws_misc, 2 * sizeof(unsigned long long));
  if (rc != GNX_OK) return rc;
  unsigned long long* derr = (unsigned long long*)ctx->ws_misc.p;
  HIPCHK(ctx, hipMemsetAsync(derr, 0xFF, 2 * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_sim_check_tables, dim3((unsigned)((N + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0, ctx->stream,
                     d_seg_off, d_seg_begin, d_seg_src, d_anc_of_src, n_founder_haps, A, C, N, derr);
  HIPCHK(ctx, hipGetLastError());
  const int64_t tiles = (C + SIM_TILE - 1) / SIM_TILE;
  hipLaunchKernelGGL(k_sim_check_founders, dim3((unsigned)tiles, (unsigned)std::min<int64_t>(n_founder_haps, SIM_MAX_GRID_Y)),
                     dim3(SIM_THREADS), 0, ctx->stream, dF, n_founder_haps, ldf, C, d_anc_of_src, A, derr);
  HIPCHK(ctx, hipGetLastError());
  unsigned long long herr[2];
  HIPCHK(ctx, hipMemcpyAsync(herr, derr, sizeof herr, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (herr[0] != ~0ull) {
    static const char* why[] = {"", "no segment", "first begin is not 0", "begins do not increase or reach C",
                                "source outside [0, n_founder_haps)", "source is not a founder (its ancestry code is >= A)"};
    return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: segment table of haplotype " + std::to_string(herr[0] >> 3) + ": " + why[herr[0] & 7]);
  }
  if (herr[1] != ~0ull) {
    const int64_t r = (int64_t)(herr[1] / (unsigned long long)C), c = (int64_t)(herr[1] % (unsigned long long)C);
    int8_t v = 0;
    HIPCHK(ctx, hipMemcpy(&v, dF + r * ldf + c, 1, hipMemcpyDeviceToHost));
    return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: founder haplotype " + std::to_string(r) + " (sample " + std::to_string(r / 2) +
                                         ") holds " + std::to_string((int)v) + " at SNP " + std::to_string(c) + ": founders must be 0 or 1");
  }
  SimArgs a{dF, n_founder_haps, ldf, C, M, C / M, d_seg_off, d_seg_begin, d_seg_src, d_anc_of_src, A, N, dX, ldx, dY, d_anc};
  const int64_t gx = std::max<int64_t>(tiles, (a.W + SIM_THREADS - 1) / SIM_THREADS);
  hipLaunchKernelGGL(k_sim_admix, dim3((unsigned)gx, (unsigned)std::min<int64_t>(N, SIM_MAX_GRID_Y)), dim3(SIM_THREADS), 0, ctx->stream, a);
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

namespace {
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

extern "C" int gnx_simulate_admix(gnx_ctx* ctx, const int8_t* F, int64_t n_founder_haps, int64_t ldf, int64_t C, int64_t M,
                                  const int64_t* seg_off, const int32_t* seg_begin, const int32_t* seg_src, const uint8_t* anc_of_src,
                                  int32_t A, int64_t N, int8_t* X, int64_t ldx, int32_t* Y, uint8_t* anc) {
  if (!ctx) return GNX_EINVAL;
  if (N < 0 || C < 1 || C > INT32_MAX || M < 1 || M > C || n_founder_haps < 1 || ldf < C || ldx < C || A < 1 || A > GNX_SIM_MAX_A)
    return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: bad arguments (need N >= 0, 1 <= M <= C < 2^31, n_founder_haps >= 1, ldf >= C, "
                                     "ldx >= C, 1 <= A <= " + std::to_string(GNX_SIM_MAX_A) + ")");
  if (N == 0) return GNX_OK;
  if (!F || !seg_off || !seg_begin || !seg_src || !anc_of_src || !X || !Y) return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: NULL array");
  // the tables' length comes from the host offsets: checked here before anything is staged
  if (seg_off[0] != 0) return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: seg_off[0] must be 0");
  for (int64_t n = 0; n < N; ++n)
    if (seg_off[n + 1] <= seg_off[n])
      return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: haplotype " + std::to_string(n) + " has no segment (seg_off must increase)");
  const int64_t S = seg_off[N], W = C / M, ld = (C + 15) / 16 * 16;   // device rows 16-byte aligned: the vector path everywhere
  if (S > INT32_MAX) return gnx_fail(ctx, GNX_EINVAL, "simulate_admix: more than 2^31 - 1 segments");
  const size_t bF = up256((size_t)n_founder_haps * ld), bX = up256((size_t)N * ld), bY = up256((size_t)N * W * 4),
               bA = anc ? up256((size_t)N * C) : 0, bOff = up256((size_t)(N + 1) * 8), bSeg = up256((size_t)S * 4),
               bAnc = up256((size_t)n_founder_haps);
  GNX_BIND_DEVICE(ctx);
  gnx_dev_tmp blk;  // the staging buffers, freed on every return
  hipError_t e = blk.alloc(bF + bX + bY + bA + bOff + 2 * bSeg + bAnc);
  if (e != hipSuccess) {
    blk.p = nullptr;
    return gnx_fail(ctx, GNX_ENOMEM, std::string("simulate_admix: hipMalloc: ") + hipGetErrorString(e));
  }
  char* p = (char*)blk.p;
  int8_t* dF = (int8_t*)p; p += bF;
  int8_t* dX = (int8_t*)p; p += bX;
  int32_t* dY = (int32_t*)p; p += bY;
  uint8_t* dA = anc ? (uint8_t*)p : nullptr; p += bA;
  int64_t* dOff = (int64_t*)p; p += bOff;
  int32_t* dBeg = (int32_t*)p; p += bSeg;
  int32_t* dSrc = (int32_t*)p; p += bSeg;
  uint8_t* dAof = (uint8_t*)p;
  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipMemcpy2DAsync(dF, ld, F, ldf, C, n_founder_haps, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dOff, seg_off, (N + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dBeg, seg_begin, S * 4, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dSrc, seg_src, S * 4, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dAof, anc_of_src, n_founder_haps, hipMemcpyHostToDevice, s));
  int rc = gnx_simulate_admix_dev(ctx, dF, n_founder_haps, ld, C, M, dOff, dBeg, dSrc, dAof, A, N, dX, ld, dY, dA);
  if (rc != GNX_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIPCHK(ctx, hipMemcpy2DAsync(X, ldx, dX, ld, C, N, hipMemcpyDeviceToHost, s));
  if (W > 0) HIPCHK(ctx, hipMemcpyAsync(Y, dY, (size_t)N * W * 4, hipMemcpyDeviceToHost, s));
  if (anc) HIPCHK(ctx, hipMemcpyAsync(anc, dA, (size_t)N * C, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}
