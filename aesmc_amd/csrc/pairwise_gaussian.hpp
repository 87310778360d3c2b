// What the pairwise Gaussian kernels share (K21, backward_sample.hip; K22, pairwise_lse.hip): the score of a particle
// (column) against a tile of points held in LDS, and the staging of that tile.  ONE definition of the score, so that it
// has the same bits wherever it is formed — K21 rests on that: the particle that holds a trajectory's maximum must have
// w == 1 exactly both in the chunk sums (N = kTile) and in the rescan of one chunk (N = 1).
#pragma once
#include "common.hpp"

namespace aesmc {

// s[j] = term - 1/2 sum_d ((tile[d * tile_stride + j] - x[d * stride_d]) * inv[d])^2 for j < N: d ascending, the scaled
// difference squared into a fused multiply-add, every j's chain independent of N and of its neighbours.
template <typename T, int N>
__device__ __forceinline__ void gaussian_scores(const T *x, int64_t stride_d, const double *tile, int tile_stride,
                                                const double *inv, int D, double term, double (&s)[N]) {
  double q[N];
#pragma unroll
  for (int j = 0; j < N; ++j) q[j] = 0.0;
  for (int d = 0; d < D; ++d) {
    const double l = (double)x[(int64_t)d * stride_d];
    const double iv = inv[d];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double diff = (tile[d * tile_stride + j] - l) * iv;
      q[j] = __builtin_fma(diff, diff, q[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) s[j] = __builtin_fma(-0.5, q[j], term);
}

// The tile's N points r0 .. r0 + N - 1 of `points` (the batch row's; one beyond R repeats the last one and is never
// written) as tile[d * N + j], and inv[d] = 1 / scale[d], both float64 in LDS; ends with the barrier.
template <typename T, int N>
__device__ __forceinline__ void stage_tile(const T *points, int64_t stride_r, int64_t stride_d, int r0, int R,
                                           const T *scale, int64_t scale_stride, int D, int tid, int threads,
                                           double *tile, double *inv) {
  for (int i = tid; i < D * N; i += threads) {
    const int d = i / N, j = i % N;
    const int r = min(r0 + j, R - 1);
    tile[i] = (double)points[(int64_t)r * stride_r + (int64_t)d * stride_d];
  }
  for (int d = tid; d < D; d += threads) inv[d] = 1.0 / (double)scale[(int64_t)d * scale_stride];
  __syncthreads();
}

}  // namespace aesmc
