// gnx_svc_rbf.h — what the RBF SVC base (k_base_rbf.hip) shares with the SVC trainer (k_train_svc.hip) and the CovRSK base
// (k_base_covrsk.hip)
#pragma once
#include "../gnx_internal.h"

#if defined(__HIPCC__)
// position of the class pair (i, j), i < j, in libsvm's order of the A (A - 1) / 2 pairwise problems
__device__ __forceinline__ int pair_index(int i, int j, int A) { return i * (2 * A - i - 1) / 2 + (j - i - 1); }
#endif

// T[k] = exp(-gamma * k), k = 0 .. n-1, with the HOST C library's exp: libsvm's kernel value for the integer squared distance k,
// as the same host's scikit-learn computes it
void gnx_rbf_table(double gamma, int64_t n, std::vector<double>& out);
// largest squared distance of two rows of `width` codes in 0..3
inline int64_t gnx_rbf_table_len(int64_t width) { return 9 * width + 1; }

// Training Gram of a batch of windows.
//   stage: X (N, ldx) int8 -> xw (nb, Np, kp): window w_first + wl's reflect-padded slice of row n, zero beyond its width and for
//          rows n >= N (Np = N rounded up to 64, kp = the widest window rounded up to 64), and nrm (nb, Np) = |row|^2
//   gram:  d2 (nb, N, N) int32 = |x_i - x_j|^2 on the int8 matrix cores, gram (nb, N, N) = (float) tab[min(d2, tmax)]
hipError_t gnx_launch_rbf_stage(const int8_t* X, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t ctx, int w_first, int nb, int W,
                                int rem, int64_t Np, int kp, int8_t* xw, int32_t* nrm, hipStream_t s);
hipError_t gnx_launch_rbf_gram(const int8_t* xw, const int32_t* nrm, int64_t N, int64_t Np, int kp, int nb, const double* tab,
                               int32_t tmax, float* gram, int32_t* d2, hipStream_t s);
