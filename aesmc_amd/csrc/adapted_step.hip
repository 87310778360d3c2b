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
// (the view, the staging helpers and the host-side checks are shared with the adjoints: adapted_step.hpp)
#include "adapted_step.hpp"

namespace aesmc {

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
