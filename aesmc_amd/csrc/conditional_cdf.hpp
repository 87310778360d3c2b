// What the conditional-resampling kernels share (conditional_ancestor_index.hip: K26; switching_conditional.hip: K37): the
// contract's running sum, added strictly front to back by ONE lane, and the bisection of a fixed number of probes over it.
#pragma once
#include "common.hpp"

namespace aesmc {

// c[j] <- c[0] + ... + c[j], added one at a time in this order (the contract's sum), by the calling lane; returns the total.
// Runs of eight are loaded ahead of the additions that wait for one another.
__device__ __forceinline__ double running_sum_in_place(double *c, int K) {
  constexpr int kRun = 8;
  double run = 0.0;
  int k = 0;
  for (; k + kRun <= K; k += kRun) {
    double w[kRun];
#pragma unroll
    for (int i = 0; i < kRun; ++i) w[i] = c[k + i];
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      run += w[i];
      c[k + i] = run;
    }
  }
  for (; k < K; ++k) {
    run += c[k];
    c[k] = run;
  }
  return run;
}

// #{ j < n : c[j] <= thr } for non-decreasing c: a fixed number of probes, strides top, top / 2, ..., 1
__device__ __forceinline__ int count_not_above(const double *c, int n, double thr, int top) {
  int pos = 0;
  for (int step = top; step > 0; step >>= 1) {
    const int probe = pos + step;
    if (probe <= n && c[probe - 1] <= thr) pos = probe;
  }
  return pos;
}

// the bisection's first stride for a row of K: 2^(ceil(log2 K) - 1) (0: K == 1)
static inline int bisection_top(int64_t K) {
  int top = 0;
  if (K > 1) {
    top = 1;
    while ((int64_t)top * 2 < K) top *= 2;
  }
  return top;
}

}  // namespace aesmc
