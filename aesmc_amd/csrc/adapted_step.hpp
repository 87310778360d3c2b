// What the launches of a fully adapted step share — the forward pair (adapted_step.hip: K27, K28) and their adjoints
// (adapted_step_backward.hip: K29, K30): the [B,K,D] view, the staging of the small float64 operands in LDS, a lane's read
// of its own row through a view, and the host side's view, alignment and size checks and the dispatch over padded extents.
#pragma once
#include "linear_gaussian.hpp"

namespace aesmc {

constexpr int kAdaptedTile = kLgBlock;      // particles per workgroup

// A [B,K,D] view by element strides, as the kernels take it
template <typename T> struct AdaptedView {
  const T *ptr;
  int64_t sb, sk, sd;
  int dense;      // [B,K,D] contiguous from a 16-byte-aligned base: the tile route
  int pairs;      // float rows that may be read in 8-byte pieces (sd == 1, every row start 8-byte aligned)
};

static inline int adapted_pad_dim(int64_t d) { return d <= 4 ? 4 : d <= 10 ? 10 : 16; }
// batch rows a tile of kAdaptedTile consecutive particles can touch — the extent of the LDS table of their offsets; 0 for
// K < 8 (more than 34 rows per tile: each lane then reads its own row's offsets, a case no filter is timed at)
static inline int64_t adapted_table_rows(int64_t K) { return K < 8 ? 0 : (kAdaptedTile - 1) / K + 2; }

// m[j * DP + i] = (j < rows && i < cols && (!lower || i <= j)) ? src[j * cols + i] : 0, for j < kLgMaxDim
template <int DP>
__device__ __forceinline__ void adapted_stage_matrix(const double *__restrict__ src, int rows, int cols, bool lower,
                                                     double *__restrict__ m) {
  for (int e = threadIdx.x; e < kLgMaxDim * DP; e += kLgBlock) {
    const int j = e / DP, i = e - j * DP;
    m[e] = (j < rows && i < cols && (!lower || i <= j)) ? src[j * cols + i] : 0.0;
  }
}

// tab[r * DP + j] = offset[b0 + r, j] for the batch rows b0 .. b0 + nrows - 1 of a tile (j < d)
template <int DP>
__device__ __forceinline__ void adapted_stage_offsets(const double *__restrict__ offset, uint32_t b0, uint32_t nrows, int d,
                                                      double *__restrict__ tab) {
  for (uint32_t e = threadIdx.x; e < nrows * (uint32_t)d; e += kLgBlock) {
    const uint32_t r = e / (uint32_t)d, j = e - r * (uint32_t)d;
    tab[r * DP + j] = offset[(int64_t)(b0 + r) * d + j];
  }
}

// One particle's row through the view, by its own lane, as float64 (columns d .. DP-1: zero)
template <typename T, int DP>
__device__ __forceinline__ void adapted_load_row(const AdaptedView<T> &v, int64_t b, int64_t k, int d, double (&x)[DP]) {
  const T *row = v.ptr + b * v.sb + k * v.sk;
  if constexpr (sizeof(T) == 4) {
    if (v.pairs) {
      const float2 *row2 = reinterpret_cast<const float2 *>(row);
#pragma unroll
      for (int i = 0; i < DP; i += 2) {
        if (i + 1 < d) {
          const float2 p = row2[i / 2];
          x[i] = (double)p.x;
          x[i + 1] = (double)p.y;
        } else {
          x[i] = i < d ? (double)row[i] : 0.0;
          if (i + 1 < DP) x[i + 1] = 0.0;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < DP; ++i) x[i] = i < d ? (double)row[(int64_t)i * v.sd] : 0.0;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static inline bool adapted_aligned(const void *p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

template <typename T>
static AdaptedView<T> adapted_view(const aesmc_view3 *v, int64_t K, int64_t D) {
  AdaptedView<T> out;
  out.ptr = (const T *)v->ptr;
  out.sb = v->stride_b, out.sk = v->stride_k, out.sd = v->stride_d;
  out.dense = (D == 1 || out.sd == 1) && out.sk == D && out.sb == K * D && adapted_aligned(v->ptr, 16);
  out.pairs = sizeof(T) == 4 && (D == 1 || out.sd == 1) && out.sk % 2 == 0 && out.sb % 2 == 0 && adapted_aligned(v->ptr, 8);
  if (D == 1) out.sd = 1;      // (one value per row: its stride is never applied)
  return out;
}

#define ADAPTED_DISPATCH(KERNEL, T, dp, grid, lds, stream, ...)                                                  \
  do {                                                                                                           \
    if ((dp) == 4) hipLaunchKernelGGL((KERNEL<T, 4>), grid, dim3(kLgBlock), lds, stream, __VA_ARGS__);           \
    else if ((dp) == 10) hipLaunchKernelGGL((KERNEL<T, 10>), grid, dim3(kLgBlock), lds, stream, __VA_ARGS__);    \
    else hipLaunchKernelGGL((KERNEL<T, 16>), grid, dim3(kLgBlock), lds, stream, __VA_ARGS__);                    \
  } while (0)

// what the entries ask of a `loc` view: a base aligned to its element, extents within 32-bit element arithmetic
static inline bool adapted_view_aligned(const aesmc_view3 *v, int dtype) {
  return adapted_aligned(v->ptr, dtype == AESMC_F32 ? 4 : 8);
}
static inline bool adapted_sizes_ok(int64_t B, int64_t K, int64_t widest) {
  return B <= 0x7fffffffLL && K <= 0x7fffffffLL && B * K <= 0x7fffffffLL / widest;
}

}  // namespace aesmc
