// The adjoints of the two launches of a fully adapted step (adapted_step.hip) — aesmc_affine_quadratic_logweight_backward
// (K29, of K27) and aesmc_adapted_draw_backward (K30, of K28) of include/aesmc_hip.h.
//
//   K29  rho[b,k,j] = o[b,j] + sum_i P[j,i] mu[b,k,i]   (K27's own chain),   w[b,k,j] = -(g[b,k] rho[b,k,j])
//        grad_loc[b,k,i] = sum_j w_j P[j,i]      grad_P[j,i] = sum_{b,k} w_j mu_i      grad_offset[b,j] = sum_k w_j
//   K30  with a = idx[b,k] (NULL: k)
//        h[b,k,i] = sum_j G[b,k,j] M[j,i]        grad_M[j,i] = sum_{b,k} G_j mu[b,a,i]  grad_r[b,j] = sum_k G_j
//                                                grad_L[j,i] = sum_{b,k} G_j eps_i  (i <= j; exactly 0 above)
//
// Geometry: K27 / K28's — 256-particle tiles of the flattened [B K] range, one lane per particle, the matrix in LDS read
// as broadcasts, dense [np, D] blocks through an LDS tile with 16-byte accesses (K29's locations, which grad_loc
// replaces; K30's arriving gradient, which h replaces), strided views and gathered rows read by their lane.  A fixed
// grid of at most kAdaptedGroups workgroups walks the tiles blockIdx.x, blockIdx.x + grid, ...
//
//   chains     grad_loc / h: ONE chain of float64 fused multiply-adds over j ascending from zero, rounded once to T.
//   matrices   every lane parks its left vector (w or G: 16 columns) and its right vectors (mu; mu[a] and eps) in LDS as
//              float64 rows of odd stride; each wavefront contracts ITS 64 particles on the float64 matrix cores —
//              16 steps of v_mfma_f64_16x16x4_f64 per matrix (A = left[particle 4 s + (l >> 4)][l & 15], B =
//              right[the same particle][l & 15], result (j, i) = ((l >> 4) + 4 reg, l & 15)) — into an accumulator quad
//              that lives across the workgroup's tiles.  At the end the four wavefronts' quads are added in wavefront
//              order and stored as the workgroup's partial; the finishing launch adds the partials in a fixed order
//              (four interleaved slices of the workgroups, each ascending, then the slices in order).
//   row sums   the same instruction with B = the indicator of a batch row: column s of the result is the sum of the left
//              vectors of the wavefront's particles in batch row (first row of the wavefront) + s, 16 rows per pass
//              (one pass whenever K >= 5).  A batch row that lies inside one wavefront's 64 particles is finished there;
//              one that crosses goes to the workspace — slot 0 of the 64-particle chunk when the row is the chunk's first,
//              slot 1 otherwise — and the finishing launch adds a row's chunks in ascending order.
//   No floating-point atomics; every sum has one fixed order for given extents: the same operands give the same bits.
//
// An index outside [0, K): that particle's left and right vectors are zeros (it contributes nothing), its h row is NaN,
// AESMC_FLAG_INDEX_OUT_OF_RANGE is raised (K28's convention).
//
// Workspace (float64): [kAdaptedGroups][2][256] matrix partials, then [4 * tiles][2][16] row partials.
#include "adapted_step.hpp"

namespace aesmc {

constexpr int kAdaptedGroups = 512;           // workgroups of a backward launch at most: two per compute unit of an MI355X
constexpr int kAdaptedLeftStride = 17;        // float64 per parked left vector (16 columns, odd stride)
constexpr int kAdaptedChunk = kWave;          // particles whose row sums one wavefront forms
typedef double adapted_quad __attribute__((ext_vector_type(4)));

template <typename T> struct QuadraticBackwardArgs {
  AdaptedView<T> loc;
  const double *P, *offset;
  const T *grad;
  T *grad_loc;                 // nullptr: not wanted
  double *ws_matrix, *ws_rows; // nullptr: grad_P / grad_offset not wanted
  double *grad_offset;
  int64_t N, tiles;
  uint32_t K;
  int D, Dy, stream;
};

template <typename T> struct DrawBackwardArgs {
  AdaptedView<T> loc;
  const int64_t *idx;
  const double *M;
  const T *eps, *grad;
  T *h;                        // nullptr: not wanted
  double *ws_matrix, *ws_rows; // nullptr: no matrix wanted / grad_r not wanted
  double *grad_r;
  int32_t *flags;
  int64_t N, tiles;
  uint32_t K;
  int D, want_m, want_l, stream;
};

struct AdaptedFinishArgs {
  const double *ws_matrix, *ws_rows;
  double *out[2];              // the matrices [rows, cols] (nullptr: not wanted)
  int lower[2];                // exactly zero above the diagonal
  double *out_rows;            // [B, Dd] (nullptr: not wanted)
  int64_t B;
  uint32_t K;
  int rows, cols, Dd, groups;
};

// acc += left^T right over the wavefront's 64 parked particles (rows 64 wave .. 64 wave + 63; absent ones hold zeros)
template <int DP>
__device__ __forceinline__ adapted_quad adapted_contract(const double *__restrict__ left, const double *__restrict__ right,
                                                         int wave, int n, int group, adapted_quad acc) {
#pragma unroll
  for (int s = 0; s < kAdaptedChunk / 4; ++s) {
    const int q = wave * kAdaptedChunk + 4 * s + group;
    const double a = left[q * kAdaptedLeftStride + n];
    const double b = n < DP ? right[q * (DP + 1) + min(n, DP - 1)] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// the sums of the parked left vectors over each batch row of the wavefront's chunk; see the header of this file
__device__ __forceinline__ void adapted_row_sums(const double *__restrict__ left, const int *__restrict__ seg, int64_t n0,
                                                 uint32_t np, uint32_t K, int Dd, int64_t tile, double *__restrict__ out,
                                                 double *__restrict__ ws_rows) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, n = lane & 15, group = lane >> 4;
  if ((uint32_t)(wave * kAdaptedChunk) >= np) return;      // (wave-uniform)
  const uint32_t nc0 = (uint32_t)n0 + wave * kAdaptedChunk;      // (B K < 2^31: adapted_sizes_ok)
  const uint32_t npw = min((uint32_t)kAdaptedChunk, (uint32_t)n0 + np - nc0);
  const uint32_t bc0 = nc0 / K, nseg = (nc0 + npw - 1) / K - bc0 + 1;
  const int64_t chunk = tile * (kAdaptedTile / kAdaptedChunk) + wave;
  for (uint32_t s0 = 0; s0 < nseg; s0 += 16) {
    adapted_quad acc = (adapted_quad){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < kAdaptedChunk / 4; ++s) {
      const int q = wave * kAdaptedChunk + 4 * s + group;
      const double a = left[q * kAdaptedLeftStride + n];
      const double b = seg[q] == (int)(s0 + n) ? 1.0 : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    const uint32_t s = s0 + n;
    if (s < nseg) {
      const uint32_t b = bc0 + s;
      const int64_t first = (int64_t)b * K;
      const bool inside = first >= (int64_t)nc0 && first + K <= (int64_t)nc0 + npw;
      double *to = inside ? out + (int64_t)b * Dd : ws_rows + (chunk * 2 + (s == 0 ? 0 : 1)) * 16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int j = group + 4 * reg;
        if (j < Dd) to[j] = acc[reg];
      }
    }
  }
}

// the workgroup's partial of one matrix: its four wavefronts' quads added in wavefront order.  `park`: 4 * 256 float64
// of LDS nobody else uses between the two barriers.
__device__ __forceinline__ void adapted_store_partial(adapted_quad acc, double *__restrict__ park, double *__restrict__ ws) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, n = lane & 15, group = lane >> 4;
  __syncthreads();
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) park[wave * 256 + (group + 4 * reg) * 16 + n] = acc[reg];
  __syncthreads();
  const int t = threadIdx.x;
  ws[t] = ((park[t] + park[256 + t]) + park[512 + t]) + park[768 + t];
}

// ---- K29 ---------------------------------------------------------------------------------------------------------------
// LDS: [kLgMaxDim * DP] P, [256 * 17] w, [256 * (DP + 1)] mu (float64), [256] batch-row numbers, then the tile of T
template <typename T, int DP>
__global__ __launch_bounds__(kLgBlock) void affine_quadratic_logweight_backward_kernel(const QuadraticBackwardArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char adapted_smem[];
  double *pm = reinterpret_cast<double *>(adapted_smem);
  double *left = pm + kLgMaxDim * DP;
  double *right = left + kAdaptedTile * kAdaptedLeftStride;
  int *seg = reinterpret_cast<int *>(right + kAdaptedTile * (DP + 1));
  T *tile = reinterpret_cast<T *>(seg + kAdaptedTile);
  const int D = a.D, Dy = a.Dy;
  const LgLayout l = lg_layout<T>((uint32_t)D);
  const uint32_t p = threadIdx.x;
  const int wave = p / kWave, lane = p % kWave, ln = lane & 15, lgroup = lane >> 4;
  const bool reduce_p = a.ws_matrix != nullptr, reduce_o = a.ws_rows != nullptr;
  adapted_quad acc = (adapted_quad){0.0, 0.0, 0.0, 0.0};
  adapted_stage_matrix<DP>(a.P, Dy, D, false, pm);
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int64_t n0 = t * kAdaptedTile;
    const uint32_t np = (uint32_t)min((int64_t)kAdaptedTile, a.N - n0);
    __syncthreads();      // the tile before this one is read and stored (first trip: nothing)
    if (a.loc.dense) lg_stage_rows(a.loc.ptr + n0 * D, np * (uint32_t)D, tile, l, a.stream);
    __syncthreads();
    const bool live = p < np;
    const int64_t n = n0 + p;
    double x[DP], w[kLgMaxDim];
    uint32_t b = 0;
    if (live) {
      b = (uint32_t)n / a.K;      // (B K < 2^31: adapted_sizes_ok)
      if (a.loc.dense) {
#pragma unroll
        for (int i = 0; i < DP; ++i) x[i] = i < D ? (double)tile[p * l.rs + i] : 0.0;
      } else {
        adapted_load_row<T, DP>(a.loc, b, n - (int64_t)b * a.K, D, x);
      }
      const double g = (double)a.grad[n];
      const double *off = a.offset + (int64_t)b * Dy;
#pragma unroll
      for (int j = 0; j < kLgMaxDim; ++j) {
        if (j < Dy) {      // (uniform)
          double r = off[j];
          const double *prow = pm + j * DP;
#pragma unroll
          for (int i = 0; i < DP; ++i) r = __builtin_fma(prow[i], x[i], r);
          w[j] = -(g * r);
        } else {
          w[j] = 0.0;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < DP; ++i) x[i] = 0.0;
#pragma unroll
      for (int j = 0; j < kLgMaxDim; ++j) w[j] = 0.0;
    }
    if (reduce_p || reduce_o) {
#pragma unroll
      for (int j = 0; j < kLgMaxDim; ++j) left[p * kAdaptedLeftStride + j] = w[j];
#pragma unroll
      for (int i = 0; i < DP; ++i) right[p * (DP + 1) + i] = x[i];
      seg[p] = live ? (int)(b - (uint32_t)(n0 + wave * kAdaptedChunk) / a.K) : -1;
    }
    if (a.grad_loc != nullptr && live) {
      T *row = tile + p * l.rs;
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        if (i < D) {      // (uniform)
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < kLgMaxDim; ++j)
            if (j < Dy) s = __builtin_fma(w[j], pm[j * DP + i], s);      // (uniform)
          row[i] = (T)s;
        }
      }
    }
    __syncthreads();
    if (a.grad_loc != nullptr) lg_store_rows(a.grad_loc + n0 * D, np * (uint32_t)D, tile, l);
    if (reduce_p) acc = adapted_contract<DP>(left, right, wave, ln, lgroup, acc);
    if (reduce_o) adapted_row_sums(left, seg, n0, np, a.K, Dy, t, a.grad_offset, a.ws_rows);
  }
  if (reduce_p) adapted_store_partial(acc, left, a.ws_matrix + (int64_t)blockIdx.x * 2 * 256);
}

// ---- K30 ---------------------------------------------------------------------------------------------------------------
// LDS: [kLgMaxDim * DP] M, [256 * 17] G, [256 * (DP + 1)] mu[a], [256 * (DP + 1)] eps (float64), [256] batch-row numbers,
// then the tile of the arriving gradient, which h replaces
template <typename T, int DP>
__global__ __launch_bounds__(kLgBlock) void adapted_draw_backward_kernel(const DrawBackwardArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char adapted_smem[];
  double *mm = reinterpret_cast<double *>(adapted_smem);
  double *left = mm + kLgMaxDim * DP;
  double *right_m = left + kAdaptedTile * kAdaptedLeftStride;
  double *right_l = right_m + kAdaptedTile * (DP + 1);
  int *seg = reinterpret_cast<int *>(right_l + kAdaptedTile * (DP + 1));
  T *tile = reinterpret_cast<T *>(seg + kAdaptedTile);
  const int D = a.D;
  const LgLayout l = lg_layout<T>((uint32_t)D);
  const uint32_t p = threadIdx.x;
  const int wave = p / kWave, lane = p % kWave, ln = lane & 15, lgroup = lane >> 4;
  const bool reduce_r = a.ws_rows != nullptr;
  const bool reduces = a.want_m || a.want_l || reduce_r;
  AdaptedView<T> noise;      // eps as a dense view read by its lane
  noise.ptr = a.eps;
  noise.sb = (int64_t)a.K * D, noise.sk = D, noise.sd = 1;
  noise.dense = 0;
  noise.pairs = sizeof(T) == 4 && D % 2 == 0;      // (the base is 16-byte aligned)
  adapted_quad acc_m = (adapted_quad){0.0, 0.0, 0.0, 0.0}, acc_l = acc_m;
  adapted_stage_matrix<DP>(a.M, D, D, false, mm);
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int64_t n0 = t * kAdaptedTile;
    const uint32_t np = (uint32_t)min((int64_t)kAdaptedTile, a.N - n0);
    const bool live = p < np;
    const int64_t n = n0 + p;
    int64_t anc = 0;
    uint32_t b = 0;
    if (live) {
      b = (uint32_t)n / a.K;      // (B K < 2^31: adapted_sizes_ok)
      anc = a.idx != nullptr ? a.idx[n] : n - (int64_t)b * a.K;
    }
    const bool in_range = live && anc >= 0 && anc < (int64_t)a.K;
    __syncthreads();      // the tile before this one is read and stored (first trip: nothing)
    lg_stage_rows(a.grad + n0 * D, np * (uint32_t)D, tile, l, a.stream);
    double x[DP], e[DP], g[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) x[i] = e[i] = 0.0;
    if (in_range && a.want_m) adapted_load_row<T, DP>(a.loc, b, anc, D, x);
    if (in_range && a.want_l) adapted_load_row<T, DP>(noise, b, n - (int64_t)b * a.K, D, e);
    __syncthreads();
    T *row = tile + p * l.rs;
#pragma unroll
    for (int j = 0; j < DP; ++j) g[j] = (in_range && j < D) ? (double)row[j] : 0.0;
    if (reduces) {
#pragma unroll
      for (int j = 0; j < kLgMaxDim; ++j) left[p * kAdaptedLeftStride + j] = j < DP ? g[min(j, DP - 1)] : 0.0;
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        right_m[p * (DP + 1) + i] = x[i];
        right_l[p * (DP + 1) + i] = e[i];
      }
      seg[p] = live ? (int)(b - (uint32_t)(n0 + wave * kAdaptedChunk) / a.K) : -1;
    }
    if (a.h != nullptr && live) {
      if (in_range) {
#pragma unroll
        for (int i = 0; i < DP; ++i) {
          if (i < D) {      // (uniform)
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < DP; ++j) s = __builtin_fma(g[j], mm[j * DP + i], s);
            row[i] = (T)s;
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < DP; ++i)
          if (i < D) row[i] = Num<T>::nan();
      }
    }
    if (live && !in_range) raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    __syncthreads();
    if (a.h != nullptr) lg_store_rows(a.h + n0 * D, np * (uint32_t)D, tile, l);
    if (a.want_m) acc_m = adapted_contract<DP>(left, right_m, wave, ln, lgroup, acc_m);
    if (a.want_l) acc_l = adapted_contract<DP>(left, right_l, wave, ln, lgroup, acc_l);
    if (reduce_r) adapted_row_sums(left, seg, n0, np, a.K, D, t, a.grad_r, a.ws_rows);
  }
  if (a.want_m) adapted_store_partial(acc_m, left, a.ws_matrix + (int64_t)blockIdx.x * 2 * 256);
  if (a.want_l) adapted_store_partial(acc_l, left, a.ws_matrix + ((int64_t)blockIdx.x * 2 + 1) * 256);
}

// ---- the finishing launch: partials added in workgroup order, a crossing batch row's chunks in ascending order -----------
// blocks 0, 1: the two matrices (thread = slice of the workgroups x element of the 16 x 16 accumulator); the blocks
// after them: 1024 (row, column) pairs of the row sums each
// A matrix block's 1024 threads are four slices of the workgroups (slice s adds the partials of workgroups s, s + 4, ...
// in ascending order: four times the loads in flight), added in slice order through LDS.
constexpr int kAdaptedFinishBlock = 1024, kAdaptedFinishSlices = kAdaptedFinishBlock / 256;

__global__ __launch_bounds__(kAdaptedFinishBlock) void adapted_backward_finish_kernel(const AdaptedFinishArgs a) {
  __shared__ double slices[kAdaptedFinishBlock];
  const int t = threadIdx.x;
  if (blockIdx.x < 2) {      // (block-uniform)
    double *out = a.out[blockIdx.x];
    if (out == nullptr) return;
    const int e = t % 256, slice = t / 256;
    const double *from = a.ws_matrix + (int64_t)blockIdx.x * 256 + e;
    double sum = 0.0;
#pragma unroll 8
    for (int g = slice; g < a.groups; g += kAdaptedFinishSlices) sum += from[(int64_t)g * 2 * 256];
    slices[t] = sum;
    __syncthreads();
    const int j = e / 16, i = e % 16;
    if (slice != 0 || j >= a.rows || i >= a.cols) return;
    sum = ((slices[e] + slices[256 + e]) + slices[512 + e]) + slices[768 + e];
    out[j * a.cols + i] = (a.lower[blockIdx.x] && i > j) ? 0.0 : sum;
    return;
  }
  if (a.out_rows == nullptr) return;
  const int64_t e = ((int64_t)blockIdx.x - 2) * kAdaptedFinishBlock + t;
  if (e >= a.B * a.Dd) return;
  const int64_t b = e / a.Dd;
  const int j = (int)(e - b * a.Dd);
  const int64_t first = b * a.K, c0 = first / kAdaptedChunk, c1 = (first + a.K - 1) / kAdaptedChunk;
  if (c0 == c1) return;      // the row lies inside one chunk, whose wavefront has written it
  // the row is the first of every chunk it reaches but, unless it starts on a chunk's boundary, of chunk c0
  double sum = a.ws_rows[(c0 * 2 + (first % kAdaptedChunk == 0 ? 0 : 1)) * 16 + j];
#pragma unroll 8
  for (int64_t c = c0 + 1; c <= c1; ++c) sum += a.ws_rows[c * 2 * 16 + j];
  a.out_rows[e] = sum;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static inline int64_t adapted_backward_tiles(int64_t B, int64_t K) { return (B * K + kAdaptedTile - 1) / kAdaptedTile; }
static inline size_t adapted_backward_matrix_doubles() { return (size_t)kAdaptedGroups * 2 * 256; }
static inline size_t adapted_backward_workspace(int64_t B, int64_t K) {
  return (adapted_backward_matrix_doubles() +
          (size_t)adapted_backward_tiles(B, K) * (kAdaptedTile / kAdaptedChunk) * 2 * 16) * sizeof(double);
}

// (tiles beyond 64 KiB of LDS need the opt-in, per kernel and device: linear_gaussian.hpp)
#define ADAPTED_BACKWARD_LAUNCH(KERNEL, T, DP_, grid, lds, stream, ...)                                           \
  do {                                                                                                           \
    bool lds_ok = true;                                                                                          \
    if ((lds) > 64 * 1024) {                                                                                     \
      static bool raised[64] = {};                                                                               \
      lds_ok = lg_raise_lds_limit(reinterpret_cast<const void *>(KERNEL<T, DP_>), raised);                       \
    }                                                                                                            \
    hipLaunchKernelGGL((KERNEL<T, DP_>), lds_ok ? dim3(grid) : dim3(0), dim3(kLgBlock), lds, stream, __VA_ARGS__); \
  } while (0)
#define ADAPTED_BACKWARD_DISPATCH(KERNEL, T, dp, grid, lds, stream, ...)                                          \
  do {                                                                                                           \
    if ((dp) == 4) ADAPTED_BACKWARD_LAUNCH(KERNEL, T, 4, grid, lds, stream, __VA_ARGS__);                        \
    else if ((dp) == 10) ADAPTED_BACKWARD_LAUNCH(KERNEL, T, 10, grid, lds, stream, __VA_ARGS__);                 \
    else ADAPTED_BACKWARD_LAUNCH(KERNEL, T, 16, grid, lds, stream, __VA_ARGS__);                                 \
  } while (0)

static int launch_adapted_finish(const AdaptedFinishArgs &f, hipStream_t s) {
  const bool matrices = f.out[0] != nullptr || f.out[1] != nullptr;
  if (!matrices && f.out_rows == nullptr) return AESMC_OK;
  const int64_t row_blocks = f.out_rows != nullptr ? (f.B * f.Dd + kAdaptedFinishBlock - 1) / kAdaptedFinishBlock : 0;
  hipLaunchKernelGGL(adapted_backward_finish_kernel, dim3((unsigned)(2 + row_blocks)), dim3(kAdaptedFinishBlock), 0, s, f);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

template <typename T>
static int launch_quadratic_backward(const aesmc_view3 *loc, const double *P, const double *offset, const void *grad,
                                     void *grad_loc, double *grad_P, double *grad_offset, double *ws, int64_t B, int64_t K,
                                     int64_t D, int64_t Dy, hipStream_t s) {
  QuadraticBackwardArgs<T> a;
  a.loc = adapted_view<T>(loc, K, D);
  a.P = P, a.offset = offset;
  a.grad = (const T *)grad, a.grad_loc = (T *)grad_loc;
  a.ws_matrix = grad_P != nullptr ? ws : nullptr;
  a.ws_rows = grad_offset != nullptr ? ws + adapted_backward_matrix_doubles() : nullptr;
  a.grad_offset = grad_offset;
  a.N = B * K, a.tiles = adapted_backward_tiles(B, K), a.K = (uint32_t)K;
  a.D = (int)D, a.Dy = (int)Dy;
  a.stream = stream_hint((uint64_t)a.N * (uint64_t)(2 * D + 1) * sizeof(T));
  const int dp = adapted_pad_dim(D);
  const bool with_tile = a.loc.dense || grad_loc != nullptr;
  const size_t lds = ((size_t)kLgMaxDim * dp + (size_t)kAdaptedTile * (kAdaptedLeftStride + dp + 1)) * sizeof(double) +
                     kAdaptedTile * sizeof(int) + (with_tile ? lg_tile_elems<T>(kAdaptedTile, (size_t)D) * sizeof(T) : 0);
  const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, kAdaptedGroups);
  ADAPTED_BACKWARD_DISPATCH(affine_quadratic_logweight_backward_kernel, T, dp, grid, lds, s, a);
  if (hipGetLastError() != hipSuccess) return AESMC_ERR_LAUNCH;
  AdaptedFinishArgs f = {};
  f.ws_matrix = ws, f.ws_rows = a.ws_rows;
  f.out[0] = grad_P, f.out[1] = nullptr;
  f.out_rows = grad_offset;
  f.B = B, f.K = (uint32_t)K;
  f.rows = (int)Dy, f.cols = (int)D, f.Dd = (int)Dy, f.groups = (int)grid;
  return launch_adapted_finish(f, s);
}

template <typename T>
static int launch_draw_backward(const aesmc_view3 *loc, const int64_t *idx, const double *M, const void *eps,
                                const void *grad, void *h, double *grad_M, double *grad_L, double *grad_r, int32_t *flags,
                                double *ws, int64_t B, int64_t K, int64_t D, hipStream_t s) {
  DrawBackwardArgs<T> a;
  a.loc = adapted_view<T>(loc, K, D);
  a.idx = idx;
  a.M = M;
  a.eps = (const T *)eps, a.grad = (const T *)grad, a.h = (T *)h;
  a.want_m = grad_M != nullptr, a.want_l = grad_L != nullptr;
  a.ws_matrix = (a.want_m || a.want_l) ? ws : nullptr;
  a.ws_rows = grad_r != nullptr ? ws + adapted_backward_matrix_doubles() : nullptr;
  a.grad_r = grad_r;
  a.flags = flags;
  a.N = B * K, a.tiles = adapted_backward_tiles(B, K), a.K = (uint32_t)K;
  a.D = (int)D;
  a.stream = stream_hint((uint64_t)a.N * (uint64_t)(4 * D) * sizeof(T));
  const int dp = adapted_pad_dim(D);
  const size_t lds = ((size_t)kLgMaxDim * dp + (size_t)kAdaptedTile * (kAdaptedLeftStride + 2 * (dp + 1))) * sizeof(double) +
                     kAdaptedTile * sizeof(int) + lg_tile_elems<T>(kAdaptedTile, (size_t)D) * sizeof(T);
  const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, kAdaptedGroups);
  ADAPTED_BACKWARD_DISPATCH(adapted_draw_backward_kernel, T, dp, grid, lds, s, a);
  if (hipGetLastError() != hipSuccess) return AESMC_ERR_LAUNCH;
  AdaptedFinishArgs f = {};
  f.ws_matrix = ws, f.ws_rows = a.ws_rows;
  f.out[0] = grad_M, f.out[1] = grad_L;
  f.lower[1] = 1;
  f.out_rows = grad_r;
  f.B = B, f.K = (uint32_t)K;
  f.rows = (int)D, f.cols = (int)D, f.Dd = (int)D, f.groups = (int)grid;
  return launch_adapted_finish(f, s);
}

}  // namespace aesmc

extern "C" int64_t aesmc_adapted_backward_workspace_bytes(int64_t B, int64_t K, int64_t D, int64_t Dy) {
  using namespace aesmc;
  if (B <= 0 || K <= 0 || D < 1 || Dy < 1 || D > kLgMaxDim || Dy > kLgMaxDim || !adapted_sizes_ok(B, K, kLgMaxDim)) return 0;
  return (int64_t)adapted_backward_workspace(B, K);
}

extern "C" int aesmc_affine_quadratic_logweight_backward(int dtype, const aesmc_view3 *loc, const double *P,
                                                         const double *offset, const void *grad, void *grad_loc,
                                                         double *grad_P, double *grad_offset, void *workspace,
                                                         int64_t workspace_bytes, int64_t B, int64_t K, int64_t D,
                                                         int64_t Dy, void *stream) {
  using namespace aesmc;
  if (loc == nullptr || loc->ptr == nullptr || P == nullptr || offset == nullptr || grad == nullptr || B < 0 || K < 0 ||
      D < 1 || Dy < 1 || workspace_bytes < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (grad_loc == nullptr && grad_P == nullptr && grad_offset == nullptr) return AESMC_ERR_INVALID_ARGUMENT;   // no output
  const size_t esz = dtype == AESMC_F32 ? 4 : 8;
  if (!adapted_view_aligned(loc, dtype) || !adapted_aligned(P, 8) || !adapted_aligned(offset, 8) ||
      !adapted_aligned(grad, esz) || !adapted_aligned(grad_loc, 16) || !adapted_aligned(grad_P, 8) ||
      !adapted_aligned(grad_offset, 8) || !adapted_aligned(workspace, 8))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (grad_loc == loc->ptr || grad_loc == grad || (const void *)grad_P == (const void *)P ||
      (const void *)grad_offset == (const void *)offset)
    return AESMC_ERR_INVALID_ARGUMENT;      // an output aliases an input
  if (B == 0 || K == 0) return AESMC_OK;
  if (D > kLgMaxDim || Dy > kLgMaxDim || !adapted_sizes_ok(B, K, kLgMaxDim)) return AESMC_ERR_UNSUPPORTED;
  if ((grad_P != nullptr || grad_offset != nullptr) &&
      (workspace == nullptr || (size_t)workspace_bytes < adapted_backward_workspace(B, K)))
    return AESMC_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_quadratic_backward<float>(loc, P, offset, grad, grad_loc, grad_P, grad_offset, (double *)workspace, B, K,
                                            D, Dy, s);
  return launch_quadratic_backward<double>(loc, P, offset, grad, grad_loc, grad_P, grad_offset, (double *)workspace, B, K, D,
                                           Dy, s);
}

extern "C" int aesmc_adapted_draw_backward(int dtype, const aesmc_view3 *loc, const int64_t *idx, const double *M,
                                           const void *eps, const void *grad, void *h, double *grad_M, double *grad_L,
                                           double *grad_r, int32_t *flags, void *workspace, int64_t workspace_bytes,
                                           int64_t B, int64_t K, int64_t D, void *stream) {
  using namespace aesmc;
  if (loc == nullptr || loc->ptr == nullptr || M == nullptr || eps == nullptr || grad == nullptr || B < 0 || K < 0 ||
      D < 1 || workspace_bytes < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (h == nullptr && grad_M == nullptr && grad_L == nullptr && grad_r == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  if (!adapted_view_aligned(loc, dtype) || !adapted_aligned(idx, 8) || !adapted_aligned(M, 8) ||
      !adapted_aligned(eps, 16) || !adapted_aligned(grad, 16) || !adapted_aligned(h, 16) || !adapted_aligned(grad_M, 8) ||
      !adapted_aligned(grad_L, 8) || !adapted_aligned(grad_r, 8) || !adapted_aligned(flags, 4) ||
      !adapted_aligned(workspace, 8))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (h == eps || h == grad || h == loc->ptr || (const void *)grad_M == (const void *)M ||
      (const void *)grad_L == (const void *)M || (grad_M != nullptr && grad_M == grad_L))
    return AESMC_ERR_INVALID_ARGUMENT;      // an output aliases an input, or another output
  if (B == 0 || K == 0) return AESMC_OK;
  if (D > kLgMaxDim || !adapted_sizes_ok(B, K, kLgMaxDim)) return AESMC_ERR_UNSUPPORTED;
  if ((grad_M != nullptr || grad_L != nullptr || grad_r != nullptr) &&
      (workspace == nullptr || (size_t)workspace_bytes < adapted_backward_workspace(B, K)))
    return AESMC_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_draw_backward<float>(loc, idx, M, eps, grad, h, grad_M, grad_L, grad_r, flags, (double *)workspace, B, K,
                                       D, s);
  return launch_draw_backward<double>(loc, idx, M, eps, grad, h, grad_M, grad_L, grad_r, flags, (double *)workspace, B, K, D,
                                      s);
}
