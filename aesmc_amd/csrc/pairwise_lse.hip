// Pairwise Gaussian log-sum-exp — aesmc_pairwise_lse of include/aesmc_hip.h (K22): the building block of the marginal
// particle smoother (FFBSm; Huerzeler & Kuensch 1998, Doucet, Godsill & Andrieu 2000).  For every batch row b and row
// point r
//
//   out[b,r] = row_add[b,r] + log sum_c exp( term[b,c] - 1/2 sum_d ((rows[b,r,d] - cols[b,c,d]) / scale[d])^2 )
//
// O(B R C D) and nothing of size [R,C] stored.  The arrangement is K21's (backward_sample.hip) without the draw:
//
//   workgroup = (batch row b, tile of kRows = 8 row points), ONE wavefront; the tile's vectors and the reciprocal scales
//               sit in LDS as float64 (every lane reads the same address: a broadcast), read once from memory;
//   lanes     = columns, 64 at a time, so `col_a` / `col_sub` are read coalesced and each `cols` element serves kRows
//               row points from a register tile of kRows running sums;
//   one pass  the wavefront keeps ONE reference value per row point for all of its lanes (the largest score it has met)
//             and every lane a sum of exp(s - reference).  A wavefront vote tells when a row point's reference has to
//             move (some lane met a larger score); only then is the new maximum reduced over the lanes and the lanes'
//             sums rescaled.  The 64 scores of step n hold the largest of all 64 n seen so far with probability 1 / n,
//             so a row point pays H(C / 64) = 3 - 5 rescales over a whole row, and every pair costs one score and one
//             exponential;
//   merge     the lanes' sums are added up; lane j finishes row point j.
//
// Measured beside it and kept as measurement forms behind aesmc_test_set_pairwise_lse_form (tools/pairwise_lse_bench.py;
// figures in profiles/ffbsm_pairwise_lse.txt): tiles of 16 row points, workgroups of four wavefronts (each takes every
// fourth run of 64 columns; their (reference, sum) pairs are merged through LDS) and the two-pass form (maxima first,
// then the sums: K21's passes 1 and 2).  All are slower at R = C = K: 1.07 - 1.14 x, 1.10 - 1.15 x and 1.23 - 1.41 x.
// Every form computes a score by the function K21 uses (gaussian_scores of pairwise_gaussian.hpp: d ascending,
// ((r - c) * inv) squared into a fused multiply-add).
#include "ancestor_index.hpp"
#include "pairwise_gaussian.hpp"

namespace aesmc {

constexpr int kLseMaxDim = 256;      // D the entry accepts: the row tile is kRows * D float64 of LDS (16 KiB at 8 rows)

template <typename T, int kRows, int kWaves, bool kTwoPass>
__global__ __launch_bounds__(kWaves *kWave) void pairwise_lse_kernel(const PairwiseArgs<T> a) {
  extern __shared__ __align__(16) double lds[];      // D * (kRows + 1) float64, sized by the launch
  __shared__ double wave_ref[kWaves][kRows];
  __shared__ double wave_sum[kWaves][kRows];
  __shared__ int wave_nan[4];                        // (16 bytes whatever kWaves is: the dynamic part stays aligned)
  double *tile = lds, *inv = lds + a.D * kRows;      // tile: [d][j]
  static_assert(kWaves <= 4, "wave_nan");
  constexpr int kThreads = kWaves * kWave;
  static_assert(kRows <= 32 && kRows <= kWave, "one NaN bit and one finishing lane per row point");

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t b = blockIdx.x / a.tiles;
  const int r0 = (int)(blockIdx.x % a.tiles) * kRows;

  // the tile's row points (one beyond R repeats the last one and is never written) and 1 / scale
  stage_tile<T, kRows>(a.rows + b * a.rows_b, a.rows_r, a.rows_d, r0, a.R, a.scale, a.scale_stride, a.D, tid, kThreads,
                       tile, inv);

  double ref[kRows], sum[kRows];      // ref: the same in every lane of a wavefront
  int nan_bits = 0;
#pragma unroll
  for (int j = 0; j < kRows; ++j) ref[j] = -__builtin_huge_val(), sum[j] = 0.0;

  if (kTwoPass) {      // ---- K21's pass 1: the maxima over the whole row, no exp --------------------------------------
    for (int c0 = wave * kWave; c0 < a.C; c0 += kThreads) {
      const int c = c0 + lane;
      double s[kRows];
      pairwise_scores<T, kRows>(a, tile, inv, b, min(c, a.C - 1), s);
#pragma unroll
      for (int j = 0; j < kRows; ++j) ref[j] = fmax(ref[j], s[j]);      // (a lane beyond C repeats column C - 1)
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) ref[j] = wave_max_uniform(ref[j]);
    if (kWaves > 1) {
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) wave_ref[wave][j] = ref[j];
      }
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) ref[j] = fmax(ref[j], wave_ref[w][j]);
      }
      __syncthreads();      // (wave_ref is written again below)
    }
  }

  // ---- the sums: exp(s - ref), the reference moving with the scores unless pass 1 has fixed it -------------------------
  for (int c0 = wave * kWave; c0 < a.C; c0 += kThreads) {
    const int c = c0 + lane;
    double s[kRows];
    pairwise_scores<T, kRows>(a, tile, inv, b, min(c, a.C - 1), s);
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const double sj = c < a.C ? s[j] : -__builtin_huge_val();
      nan_bits |= (sj != sj) ? (1 << j) : 0;
      if (!kTwoPass && __ballot(sj > ref[j]) != 0) {      // (wave-uniform)  some lane's score is above the reference
        const double top = wave_max_uniform(sj);
        sum[j] *= exp_nonpositive(ref[j] - top);          // (from -inf: the sums are still zero and stay so)
        ref[j] = top;
      }
      sum[j] += exp_nonpositive(sj - ref[j]);             // (NaN and -inf - -inf give 0: see exp_nonpositive's guard)
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    nan_bits |= __shfl_xor(nan_bits, off, kWave);
#pragma unroll
    for (int j = 0; j < kRows; ++j) sum[j] += __shfl_xor(sum[j], off, kWave);
  }
  if (lane == 0) {
    wave_nan[wave] = nan_bits;
#pragma unroll
    for (int j = 0; j < kRows; ++j) wave_ref[wave][j] = ref[j], wave_sum[wave][j] = sum[j];
  }
  __syncthreads();

  // ---- merge the wavefronts' pairs: lane j of the first wavefront finishes row point r0 + j -----------------------------
  if (tid < kRows && r0 + tid < a.R) {
    const int j = tid;
    double top = wave_ref[0][j];
    int nan = wave_nan[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) top = fmax(top, wave_ref[w][j]), nan |= wave_nan[w];
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += wave_sum[w][j] * exp_nonpositive(wave_ref[w][j] - top);
    const int64_t at = b * a.R + r0 + j;
    const double add = a.row_add != nullptr ? (double)a.row_add[at] : 0.0;
    double value;
    if (((nan >> j) & 1) || add != add) {
      raise_flag(a.flags, AESMC_FLAG_NAN_LOG_WEIGHT);
      value = __builtin_nan("");
    } else if (top == __builtin_huge_val()) {
      raise_flag(a.flags, AESMC_FLAG_DEGENERATE_ROW);
      value = top;
    } else if (top == -__builtin_huge_val()) {
      value = top;      // every score -inf: a point of zero weight, no flag
    } else {
      value = add + (top + ::log(total));
    }
    a.out[at] = (T)value;
  }
}

// which form a launch takes: 0 = the default of each; tools/pairwise_lse_bench.py walks the others through the test hook
static int g_lse_rows = 0, g_lse_waves = 0, g_lse_passes = 0;
constexpr int kLseDefaultRows = 8, kLseDefaultWaves = 1, kLseDefaultPasses = 1;

template <typename T, int kRows, int kWaves, bool kTwoPass>
static int launch_pairwise_form(PairwiseArgs<T> a, int64_t B, hipStream_t s) {
  a.tiles = (a.R + kRows - 1) / kRows;      // (B * tiles fits: the entry checks it for the smallest tile)
  hipLaunchKernelGGL((pairwise_lse_kernel<T, kRows, kWaves, kTwoPass>), dim3((unsigned)(B * a.tiles)),
                     dim3(kWaves * kWave), (size_t)a.D * (kRows + 1) * sizeof(double), s, a);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

template <typename T>
static int launch_pairwise_lse(const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale, int64_t scale_stride,
                               const void *col_a, const void *col_sub, const void *row_add, void *out, int32_t *flags,
                               int64_t B, int64_t R, int64_t C, int64_t D, hipStream_t s) {
  PairwiseArgs<T> a = {};
  if (D > 0) {
    a.rows = (const T *)rows->ptr;
    a.rows_b = rows->stride_b, a.rows_r = rows->stride_k, a.rows_d = rows->stride_d;
    a.cols = (const T *)cols->ptr;
    a.cols_b = cols->stride_b, a.cols_c = cols->stride_k, a.cols_d = cols->stride_d;
    a.scale = (const T *)scale;
    a.scale_stride = scale_stride;
  }
  a.col_a = (const T *)col_a, a.col_sub = (const T *)col_sub, a.row_add = (const T *)row_add;
  a.out = (T *)out;
  a.flags = flags;
  a.R = (int)R, a.C = (int)C, a.D = (int)D;
  const int rows_per = g_lse_rows ? g_lse_rows : kLseDefaultRows;
  const int waves = g_lse_waves ? g_lse_waves : kLseDefaultWaves;
  const bool two = (g_lse_passes ? g_lse_passes : kLseDefaultPasses) == 2;
#define AESMC_LSE_FORM(ROWS, WAVES)                                                              \
  if (rows_per == ROWS && waves == WAVES)                                                        \
    return two ? launch_pairwise_form<T, ROWS, WAVES, true>(a, B, s) : launch_pairwise_form<T, ROWS, WAVES, false>(a, B, s);
  AESMC_LSE_FORM(8, 4)
  AESMC_LSE_FORM(16, 4)
  AESMC_LSE_FORM(8, 1)
  AESMC_LSE_FORM(16, 1)
#undef AESMC_LSE_FORM
  return AESMC_ERR_INVALID_ARGUMENT;
}

}  // namespace aesmc

extern "C" int aesmc_pairwise_lse(int dtype, const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale,
                                  int64_t scale_stride, const void *col_a, const void *col_sub, const void *row_add,
                                  void *out, int32_t *flags, int64_t B, int64_t R, int64_t C, int64_t D, void *stream) {
  using namespace aesmc;
  if (col_a == nullptr || out == nullptr || B < 0 || R < 0 || C < 0 || D < 0) return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (D > 0 && (rows == nullptr || cols == nullptr || scale == nullptr || rows->ptr == nullptr || cols->ptr == nullptr ||
                (scale_stride != 0 && scale_stride != 1)))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || R == 0) return AESMC_OK;
  if (C == 0) return AESMC_ERR_INVALID_ARGUMENT;      // row points to sum for and no column to sum over
  if (D > kLseMaxDim) return AESMC_ERR_UNSUPPORTED;
  if (R > 0x3fffffffLL || C > 0x3fffffffLL || B > 0x7fffffffLL || B * ((R + 7) / 8) > 0x7fffffffLL)
    return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_pairwise_lse<float>(rows, cols, scale, scale_stride, col_a, col_sub, row_add, out, flags, B, R, C, D, s);
  return launch_pairwise_lse<double>(rows, cols, scale, scale_stride, col_a, col_sub, row_add, out, flags, B, R, C, D, s);
}

// Measurement / test hook (not part of include/aesmc_hip.h): the tile height (8, 16), the wavefronts per workgroup (1, 4)
// and the passes (1, 2) of the launches that follow; 0 = the default of each.
extern "C" int aesmc_test_set_pairwise_lse_form(int rows, int waves, int passes) {
  if ((rows != 0 && rows != 8 && rows != 16) || (waves != 0 && waves != 1 && waves != 4) || passes < 0 || passes > 2)
    return AESMC_ERR_INVALID_ARGUMENT;
  aesmc::g_lse_rows = rows, aesmc::g_lse_waves = waves, aesmc::g_lse_passes = passes;
  return AESMC_OK;
}
