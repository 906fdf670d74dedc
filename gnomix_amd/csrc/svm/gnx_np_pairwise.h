// gnx_np_pairwise.h — numpy's pairwise summation of float64, restated for a stream of values.
//
// np.sum over a contiguous float64 array adds in the order of DOUBLE_pairwise_sum (numpy/core/src/umath/loops_utils.h.src, third
// party): up to 128 elements in eight interleaved accumulators that are combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and then
// take the n % 8 tail one by one; above 128 elements PW(n) = PW(n2) + PW(n - n2) with n2 = n/2 rounded down to a multiple of 8.
// The polynomial string kernel (string_kernel.py:40-61: np.sum(contigs ** p) / p) is only reproduced bit for bit in that order.
// k_svc_gram_poly (the trainer's Gram pass) produces its values on the fly, so the sum takes the element COUNT and a generator
// that returns the next element; the recursion is walked with an explicit stack.  k_covrsk_dec<true> (inference, k_base_covrsk.hip)
// carries the same restatement inline: the two must stay in step, and fixture G10 pins that one to the reference's own matrix.
#pragma once

// frames of the explicit stack: a frame's size is at most n / 2^depth + 15 (the right half is the larger one and exceeds half by
// less than 8 per level), so 12 frames cover every n below 2^17 — sixteen times the widest window the Gram pass accepts
constexpr int GNX_NP_PAIRWISE_FRAMES = 12;

template <class Next>
__device__ __forceinline__ double gnx_np_pairwise_sum(int n_el, Next&& next_val) {
  auto leaf = [&](int m) -> double {  // numpy DOUBLE_pairwise_sum for n <= 128
    if (m < 8) {
      double res = 0.;
      for (int i = 0; i < m; ++i) res += next_val();
      return res;
    }
    double r0 = next_val(), r1 = next_val(), r2 = next_val(), r3 = next_val(), r4 = next_val(), r5 = next_val(),
           r6 = next_val(), r7 = next_val();
    int i = 8;
    for (; i < m - (m % 8); i += 8) {
      r0 += next_val(); r1 += next_val(); r2 += next_val(); r3 += next_val();
      r4 += next_val(); r5 += next_val(); r6 += next_val(); r7 += next_val();
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < m; ++i) res += next_val();
    return res;
  };
  // the recursion  PW(n) = PW(n2) + PW(n - n2), n2 = n/2 rounded down to a multiple of 8, n > 128, made iterative
  int fsz[GNX_NP_PAIRWISE_FRAMES], fst[GNX_NP_PAIRWISE_FRAMES];
  double flv[GNX_NP_PAIRWISE_FRAMES];
  int top = 0;
  fsz[0] = n_el; fst[0] = 0;
  double ret = 0.0;
  bool have = false;
  while (top >= 0) {
    if (!have) {
      if (fsz[top] <= 128) { ret = leaf(fsz[top]); have = true; --top; }
      else {
        int n2 = fsz[top] / 2; n2 -= n2 % 8;
        fst[top] = 0;
        fsz[top + 1] = n2; fst[top + 1] = 0;
        ++top;
      }
    } else if (fst[top] == 0) {
      flv[top] = ret; fst[top] = 1; have = false;
      int n2 = fsz[top] / 2; n2 -= n2 % 8;
      fsz[top + 1] = fsz[top] - n2; fst[top + 1] = 0;
      ++top;
    } else {
      ret = flv[top] + ret;
      --top;
    }
  }
  return ret;
}
