// The two launches of a fully adapted auxiliary particle filter step (Pitt & Shephard 1999) around the resampling launch
// (K2) — aesmc_affine_quadratic_logweight (K27) and aesmc_adapted_draw (K28) of include/aesmc_hip.h.
//
// For a Normal transition N(mu(x_{t-1}), S_f) with a constant diagonal S_f and an emission N(C x_t + d, S_g) that is linear
// in the newest latent, the predictive likelihood p(y_t | x_{t-1}) and the optimal proposal p(x_t | x_{t-1}, y_t) are
// Gaussian in closed form; the host forms their small matrices once in float64 (aesmc_amd/adapted.py, `gains`):
//
//   K27  log lambda[b,k] = base - 1/2 || P mu[b,k] + o_b ||^2                 = log p(y_t | x_{t-1}[b,k])     first stage
//   K2   a[b,:] from log lambda[b,:]                                          (the existing resampling launch)
//   K28  x_t[b,k] = r_b + M mu[b, a[b,k]] + L eps[b,k]                        ~ p(x_t | x_{t-1}[b,a], y_t)    the draw
//
//   workgroup = 256 consecutive particles of the flattened [B K] range, one lane per particle;
//   matrices  float64, zero-padded to DP columns in LDS, read as broadcasts; the offsets of the batch rows a tile touches
//             (two when K >= 256, 33 when K == 8) in an LDS table beside them;
//   rows      dense [np, D] blocks (K27's locations, K28's noise and draws) go through an LDS tile with 16-byte accesses,
//             as K8's do (40-byte rows are not 16-byte aligned: a lane cannot load its own row as vectors); a strided view
//             (particle stride 0: step 0) and K28's gathered rows are read by their lane, in 8-byte pieces where every
//             address involved allows it;
//   chains    every output is ONE chain of float64 fused multiply-adds in the header's order, rounded once to T.  The
//             padded columns multiply a zero weight by a zero element: the chain's bits do not change.  K28 is unrolled in
//             both directions, so the triangle i <= j of L is a compile-time matter and nothing above it is read.
//
// Both are streaming kernels: at B = 1024, K = 4096, D = Dy = 10, float32, K27 reads 168 MB and writes 17 MB, K28 reads
// 34 MB of indices, 168 MB of noise and the gathered rows and writes 168 MB; the ~100 / ~155 float64 multiply-adds per
// particle stay under the memory time (profiles/adapted_filter.txt).
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

template <typename T> struct QuadraticArgs {
  AdaptedView<T> loc;
  const double *P, *offset;
  double base;
  T *out;
  int64_t N;
  uint32_t K;
  int D, Dy, stream;
};

template <typename T> struct DrawArgs {
  AdaptedView<T> loc;
  const int64_t *idx;
  const double *M, *offset, *L;
  const T *eps;
  T *out;
  int32_t *flags;
  int64_t N;
  uint32_t K;
  int D, stream;
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

// ---- K27 ---------------------------------------------------------------------------------------------------------------
// LDS: [kLgMaxDim * DP] P, [table rows * kLgMaxDim] offsets (float64), then the tile of locations (dense views)
template <typename T, int DP>
__global__ __launch_bounds__(kLgBlock) void affine_quadratic_logweight_kernel(const QuadraticArgs<T> a, int table_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char adapted_smem[];
  double *pm = reinterpret_cast<double *>(adapted_smem);
  double *tab = pm + kLgMaxDim * DP;
  T *tile = reinterpret_cast<T *>(tab + (size_t)table_rows * kLgMaxDim);
  const int D = a.D, Dy = a.Dy;
  const int64_t n0 = (int64_t)blockIdx.x * kAdaptedTile;
  const uint32_t np = (uint32_t)min((int64_t)kAdaptedTile, a.N - n0);
  const uint32_t b0 = (uint32_t)(n0 / a.K), nrows = (uint32_t)((n0 + np - 1) / a.K) - b0 + 1;
  const LgLayout l = lg_layout<T>((uint32_t)D);
  adapted_stage_matrix<DP>(a.P, Dy, D, false, pm);
  if (table_rows) adapted_stage_offsets<kLgMaxDim>(a.offset, b0, nrows, Dy, tab);
  if (a.loc.dense) lg_stage_rows(a.loc.ptr + n0 * D, np * (uint32_t)D, tile, l, a.stream);
  __syncthreads();
  const uint32_t p = threadIdx.x;
  if (p >= np) return;
  const int64_t n = n0 + p;
  const uint32_t b = (uint32_t)(n / a.K), k = (uint32_t)(n - (int64_t)b * a.K);
  double x[DP];
  if (a.loc.dense) {
#pragma unroll
    for (int i = 0; i < DP; ++i) x[i] = i < D ? (double)tile[p * l.rs + i] : 0.0;
  } else {
    adapted_load_row<T, DP>(a.loc, b, k, D, x);
  }
  const double *off = table_rows ? tab + (b - b0) * kLgMaxDim : a.offset + (int64_t)b * Dy;
  double q = 0.0;
#pragma unroll 2
  for (int j = 0; j < Dy; ++j) {
    double r = off[j];
    const double *prow = pm + j * DP;
#pragma unroll
    for (int i = 0; i < DP; ++i) r = __builtin_fma(prow[i], x[i], r);
    q = __builtin_fma(r, r, q);
  }
  a.out[n] = (T)(a.base - 0.5 * q);
}

// ---- K28 ---------------------------------------------------------------------------------------------------------------
// LDS: [kLgMaxDim * DP] M, [kLgMaxDim * DP] L (zero above the diagonal), [table rows * kLgMaxDim] offsets (float64), then
// the tile of noise, which the draws replace
template <typename T, int DP>
__global__ __launch_bounds__(kLgBlock) void adapted_draw_kernel(const DrawArgs<T> a, int table_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char adapted_smem[];
  double *mm = reinterpret_cast<double *>(adapted_smem);
  double *lm = mm + kLgMaxDim * DP;
  double *tab = lm + kLgMaxDim * DP;
  T *tile = reinterpret_cast<T *>(tab + (size_t)table_rows * kLgMaxDim);
  const int D = a.D;
  const int64_t n0 = (int64_t)blockIdx.x * kAdaptedTile;
  const uint32_t np = (uint32_t)min((int64_t)kAdaptedTile, a.N - n0);
  const uint32_t b0 = (uint32_t)(n0 / a.K), nrows = (uint32_t)((n0 + np - 1) / a.K) - b0 + 1;
  const LgLayout l = lg_layout<T>((uint32_t)D);
  const uint32_t p = threadIdx.x;
  const bool live = p < np;
  const int64_t n = n0 + p;
  // the ancestor first: the gathered row's address waits for it
  int64_t anc = 0;
  uint32_t b = 0;
  if (live) {
    b = (uint32_t)(n / a.K);
    anc = a.idx != nullptr ? a.idx[n] : n - (int64_t)b * a.K;
  }
  adapted_stage_matrix<DP>(a.M, D, D, false, mm);
  adapted_stage_matrix<DP>(a.L, D, D, true, lm);
  if (table_rows) adapted_stage_offsets<kLgMaxDim>(a.offset, b0, nrows, D, tab);
  lg_stage_rows(a.eps + n0 * D, np * (uint32_t)D, tile, l, a.stream);
  const bool in_range = live && anc >= 0 && anc < (int64_t)a.K;
  double x[DP];
  if (in_range) {
    adapted_load_row<T, DP>(a.loc, b, anc, D, x);
  } else {
#pragma unroll
    for (int i = 0; i < DP; ++i) x[i] = 0.0;
  }
  __syncthreads();
  if (live) {
    T *row = tile + p * l.rs;
    if (in_range) {
      const double *off = table_rows ? tab + (b - b0) * kLgMaxDim : a.offset + (int64_t)b * D;
      double e[DP];
#pragma unroll
      for (int i = 0; i < DP; ++i) e[i] = i < D ? (double)row[i] : 0.0;
#pragma unroll
      for (int j = 0; j < DP; ++j) {
        if (j < D) {      // (uniform)
          double acc = off[j];
#pragma unroll
          for (int i = 0; i < DP; ++i) acc = __builtin_fma(mm[j * DP + i], x[i], acc);
#pragma unroll
          for (int i = 0; i <= j; ++i) acc = __builtin_fma(lm[j * DP + i], e[i], acc);
          row[j] = (T)acc;
        }
      }
    } else {
      raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
#pragma unroll
      for (int j = 0; j < DP; ++j)
        if (j < D) row[j] = Num<T>::nan();
    }
  }
  __syncthreads();
  lg_store_rows(a.out + n0 * D, np * (uint32_t)D, tile, l);
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

template <typename T>
static int launch_quadratic(const aesmc_view3 *loc, const double *P, const double *offset, double base, void *out, int64_t B,
                            int64_t K, int64_t D, int64_t Dy, hipStream_t s) {
  QuadraticArgs<T> a;
  a.loc = adapted_view<T>(loc, K, D);
  a.P = P, a.offset = offset, a.base = base;
  a.out = (T *)out;
  a.N = B * K, a.K = (uint32_t)K;
  a.D = (int)D, a.Dy = (int)Dy;
  a.stream = stream_hint((uint64_t)a.N * (uint64_t)(D + 1) * sizeof(T));
  const int dp = adapted_pad_dim(D);
  const int rows = (int)adapted_table_rows(K);
  const size_t lds = ((size_t)kLgMaxDim * dp + (size_t)rows * kLgMaxDim) * sizeof(double) +
                     (a.loc.dense ? lg_tile_elems<T>(kAdaptedTile, (size_t)D) * sizeof(T) : 0);
  const dim3 grid((unsigned)((a.N + kAdaptedTile - 1) / kAdaptedTile));
  ADAPTED_DISPATCH(affine_quadratic_logweight_kernel, T, dp, grid, lds, s, a, rows);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

template <typename T>
static int launch_draw(const aesmc_view3 *loc, const int64_t *idx, const double *M, const double *offset, const double *L,
                       const void *eps, void *out, int32_t *flags, int64_t B, int64_t K, int64_t D, hipStream_t s) {
  DrawArgs<T> a;
  a.loc = adapted_view<T>(loc, K, D);
  a.idx = idx;
  a.M = M, a.offset = offset, a.L = L;
  a.eps = (const T *)eps, a.out = (T *)out;
  a.flags = flags;
  a.N = B * K, a.K = (uint32_t)K;
  a.D = (int)D;
  a.stream = stream_hint((uint64_t)a.N * (uint64_t)(3 * D) * sizeof(T));
  const int dp = adapted_pad_dim(D);
  const int rows = (int)adapted_table_rows(K);
  const size_t lds = ((size_t)2 * kLgMaxDim * dp + (size_t)rows * kLgMaxDim) * sizeof(double) +
                     lg_tile_elems<T>(kAdaptedTile, (size_t)D) * sizeof(T);
  const dim3 grid((unsigned)((a.N + kAdaptedTile - 1) / kAdaptedTile));
  ADAPTED_DISPATCH(adapted_draw_kernel, T, dp, grid, lds, s, a, rows);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

// what the two entries ask of a `loc` view: a base aligned to its element, extents within 32-bit element arithmetic
static inline bool adapted_view_aligned(const aesmc_view3 *v, int dtype) {
  return adapted_aligned(v->ptr, dtype == AESMC_F32 ? 4 : 8);
}
static inline bool adapted_sizes_ok(int64_t B, int64_t K, int64_t widest) {
  return B <= 0x7fffffffLL && K <= 0x7fffffffLL && B * K <= 0x7fffffffLL / widest;
}

}  // namespace aesmc

extern "C" int aesmc_affine_quadratic_logweight(int dtype, const aesmc_view3 *loc, const double *P, const double *offset,
                                                double base, void *out, int64_t B, int64_t K, int64_t D, int64_t Dy,
                                                void *stream) {
  using namespace aesmc;
  if (loc == nullptr || loc->ptr == nullptr || P == nullptr || offset == nullptr || out == nullptr || B < 0 || K < 0 ||
      D < 1 || Dy < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (!adapted_view_aligned(loc, dtype) || !adapted_aligned(P, 8) || !adapted_aligned(offset, 8) ||
      !adapted_aligned(out, dtype == AESMC_F32 ? 4 : 8))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (D > kLgMaxDim || Dy > kLgMaxDim || !adapted_sizes_ok(B, K, kLgMaxDim)) return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32) return launch_quadratic<float>(loc, P, offset, base, out, B, K, D, Dy, s);
  return launch_quadratic<double>(loc, P, offset, base, out, B, K, D, Dy, s);
}

extern "C" int aesmc_adapted_draw(int dtype, const aesmc_view3 *loc, const int64_t *idx, const double *M,
                                  const double *offset, const double *L, const void *eps, void *out, int32_t *flags,
                                  int64_t B, int64_t K, int64_t D, void *stream) {
  using namespace aesmc;
  if (loc == nullptr || loc->ptr == nullptr || M == nullptr || offset == nullptr || L == nullptr || eps == nullptr ||
      out == nullptr || B < 0 || K < 0 || D < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (!adapted_view_aligned(loc, dtype) || !adapted_aligned(idx, 8) || !adapted_aligned(M, 8) ||
      !adapted_aligned(offset, 8) || !adapted_aligned(L, 8) || !adapted_aligned(eps, 16) || !adapted_aligned(out, 16) ||
      !adapted_aligned(flags, 4) || out == eps || out == loc->ptr)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (D > kLgMaxDim || !adapted_sizes_ok(B, K, kLgMaxDim)) return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32) return launch_draw<float>(loc, idx, M, offset, L, eps, out, flags, B, K, D, s);
  return launch_draw<double>(loc, idx, M, offset, L, eps, out, flags, B, K, D, s);
}
