// What the pairwise Gaussian kernels share (K21, backward_sample.hip; K22, pairwise_lse.hip; K23, pairwise_mean.hip): the
// score of a particle (column) against a tile of points held in LDS, and the staging of that tile.  ONE definition of the
// score, so that it has the same bits wherever it is formed — K21 rests on that: the particle that holds a trajectory's
// maximum must have w == 1 exactly both in the chunk sums (N = kTile) and in the rescan of one chunk (N = 1).
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

// ---- what the pairwise kernels over [B,R] x [B,C] share (K22, pairwise_lse.hip; K23, pairwise_mean.hip) ----------------
template <typename T> struct PairwiseArgs {
  const T *rows, *cols, *scale;
  int64_t rows_b, rows_r, rows_d, cols_b, cols_c, cols_d, scale_stride;
  const T *col_a, *col_sub, *row_add;
  T *out;
  int32_t *flags;
  int R, C, D, tiles;
};

// s[j] for the tile's kRows row points and column c of batch row b
template <typename T, int kRows>
__device__ __forceinline__ void pairwise_scores(const PairwiseArgs<T> &a, const double *tile, const double *inv, int64_t b,
                                                int c, double (&s)[kRows]) {
  const int64_t at = b * a.C + c;
  double term = (double)a.col_a[at];
  if (a.col_sub != nullptr) {      // (launch-uniform)  an absent column stays absent whatever col_sub holds
    const double sub = (double)a.col_sub[at];
    term = term == -__builtin_huge_val() ? term : term - sub;
  }
  gaussian_scores<T, kRows>(a.cols + b * a.cols_b + (int64_t)c * a.cols_c, a.cols_d, tile, kRows, inv, a.D, term, s);
}

// the largest x of the wavefront (fmax drops a NaN operand), held in scalar registers: the same in every lane
__device__ __forceinline__ double wave_max_uniform(double x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, kWave));
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  return __hiloint2double(hi, lo);
}

}  // namespace aesmc
