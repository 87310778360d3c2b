// Pairwise Gaussian max and argmax — aesmc_pairwise_argmax of include/aesmc_hip.h (K24): the building block of the MAP
// trajectory (the particle Viterbi recursion of Godsill, Doucet & West 2001).  For every batch row b and row point r, with
// s[r,c] the score K22 sums (pairwise_lse.hip)
//
//   out[b,r] = row_add[b,r] + max_c s[r,c]          arg[b,r] = the smallest c that attains the maximum
//
// the max-plus twin of K22: O(B R C D) and nothing of size [R,C] stored.  The arrangement is K22's without the
// exponentials, and without its moving reference (a maximum needs none):
//
//   workgroup = (batch row b, tile of kArgRows = 8 row points), ONE wavefront; the tile's vectors and the reciprocal
//               scales sit in LDS as float64 (every lane reads the same address: a broadcast), read once from memory;
//   lanes     = columns, 64 at a time; every lane keeps, per row point, the best score it has met and that score's
//               column.  Its columns ascend, so a strict `>` keeps the smallest column of the lane's best score;
//   merge     one butterfly over the lanes of (score, column) pairs: the larger score wins, equal scores take the smaller
//               column — with the lanes' own rule that is the smallest column of the whole row, whatever lane and chunk the
//               tied columns sit in.  Lane j finishes row point j.
//
// Ties are exact: a column's score chain (gaussian_scores of pairwise_gaussian.hpp) does not depend on its lane or its
// neighbours, so columns with identical operands have identical bits.  A NaN score never enters a lane's best (the
// comparison is false); it is carried by a wavefront vote per row point, OR-ed into scalar registers: the vector pipe pays
// the comparison alone, and the bits need no merge.
//
// Per pair the loop costs the score's 3 D + 1 float64 operations, two compares and three selects (the score's two words
// and the column); K22 pays an exponential there.  The last chunk needs no mask: a lane beyond C repeats column
// C - 1 under that column's own index, and a pair met twice changes neither the maximum nor its smallest column.
//
// Resources (the compiler's resource report, the same for float32 and float64 operands): 72 VGPR, 7 wavefronts per
// SIMD, no scratch, LDS = 96 bytes static + 72 D bytes for the tile and the reciprocal scales.
#include "pairwise_gaussian.hpp"

namespace aesmc {

constexpr int kArgMaxDim = 256;      // D the entry accepts: the row tile is kArgRows * D float64 of LDS (16 KiB)
constexpr int kArgRows = 8;          // row points per workgroup

template <typename T>
__global__ __launch_bounds__(kWave) void pairwise_argmax_kernel(const PairwiseArgs<T> a, int64_t *arg) {
  constexpr int kRows = kArgRows;
  extern __shared__ __align__(16) double lds[];      // D * (kRows + 1) float64, sized by the launch
  __shared__ double fin_best[kRows];
  __shared__ int fin_at[kRows];
  double *tile = lds, *inv = lds + a.D * kRows;      // tile: [d][j]
  static_assert(kRows <= 32 && kRows <= kWave, "one NaN bit and one finishing lane per row point");

  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / a.tiles;
  const int r0 = (int)(blockIdx.x % a.tiles) * kRows;

  // the tile's row points (one beyond R repeats the last one and is never written) and 1 / scale
  stage_tile<T, kRows>(a.rows + b * a.rows_b, a.rows_r, a.rows_d, r0, a.R, a.scale, a.scale_stride, a.D, lane, kWave, tile,
                       inv);

  double best[kRows];
  int at[kRows];                      // C: no column yet (nothing above -inf has been met)
  uint64_t nan_lanes[kRows];          // the lanes that have met a NaN score: a wavefront vote, held in scalar registers
#pragma unroll
  for (int j = 0; j < kRows; ++j) best[j] = -__builtin_huge_val(), at[j] = a.C, nan_lanes[j] = 0;

  for (int c0 = 0; c0 < a.C; c0 += kWave) {
    const int c = min(c0 + lane, a.C - 1);      // a lane beyond C repeats column C - 1 under its own index: harmless twice
    double s[kRows];
    pairwise_scores<T, kRows>(a, tile, inv, b, c, s);
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      nan_lanes[j] |= __builtin_amdgcn_ballot_w64(s[j] != s[j]);      // (the compare's own mask)
      const bool better = s[j] > best[j];                            // (false for a NaN, and for -inf over -inf)
      best[j] = better ? s[j] : best[j];
      at[j] = better ? c : at[j];
    }
  }

  // ---- the lanes' pairs are merged: larger score, then smaller column; every lane ends with the row's pair -----------------
  int nan_bits = 0;                   // (wave-uniform)
#pragma unroll
  for (int j = 0; j < kRows; ++j) nan_bits |= nan_lanes[j] != 0 ? (1 << j) : 0;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const double other = __shfl_xor(best[j], off, kWave);
      const int other_at = __shfl_xor(at[j], off, kWave);
      const bool take = (other > best[j]) | ((other == best[j]) & (other_at < at[j]));      // (no branches)
      best[j] = take ? other : best[j];
      at[j] = take ? other_at : at[j];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kRows; ++j) fin_best[j] = best[j], fin_at[j] = at[j];
  }
  __syncthreads();

  // ---- lane j finishes row point r0 + j -----------------------------------------------------------------------------------
  if (lane < kRows && r0 + lane < a.R) {
    const int j = lane;
    const double top = fin_best[j];
    const int64_t at_row = b * a.R + r0 + j;
    const double add = a.row_add != nullptr ? (double)a.row_add[at_row] : 0.0;
    double value;
    int64_t column = a.C;      // "no column" unless the maximum is finite
    if (((nan_bits >> j) & 1) || add != add) {
      raise_flag(a.flags, AESMC_FLAG_NAN_LOG_WEIGHT);
      value = __builtin_nan("");
    } else if (top == __builtin_huge_val()) {
      raise_flag(a.flags, AESMC_FLAG_DEGENERATE_ROW);
      value = top;
    } else if (top == -__builtin_huge_val()) {
      value = top;      // every score -inf: a point nothing reaches, no flag
    } else {
      value = add + top;
      column = fin_at[j];
    }
    a.out[at_row] = (T)value;
    if (arg != nullptr) arg[at_row] = column;
  }
}

template <typename T>
static int launch_pairwise_argmax(const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale, int64_t scale_stride,
                                  const void *col_a, const void *col_sub, const void *row_add, void *out, int64_t *arg,
                                  int32_t *flags, int64_t B, int64_t R, int64_t C, int64_t D, hipStream_t s) {
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
  a.tiles = (a.R + kArgRows - 1) / kArgRows;      // (B * tiles fits: the entry checks it)
  hipLaunchKernelGGL((pairwise_argmax_kernel<T>), dim3((unsigned)(B * a.tiles)), dim3(kWave),
                     (size_t)a.D * (kArgRows + 1) * sizeof(double), s, a, arg);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc

extern "C" int aesmc_pairwise_argmax(int dtype, const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale,
                                     int64_t scale_stride, const void *col_a, const void *col_sub, const void *row_add,
                                     void *out, int64_t *arg, int32_t *flags, int64_t B, int64_t R, int64_t C, int64_t D,
                                     void *stream) {
  using namespace aesmc;
  if (col_a == nullptr || out == nullptr || B < 0 || R < 0 || C < 0 || D < 0) return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (D > 0 && (rows == nullptr || cols == nullptr || scale == nullptr || rows->ptr == nullptr || cols->ptr == nullptr ||
                (scale_stride != 0 && scale_stride != 1)))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || R == 0) return AESMC_OK;
  if (C == 0) return AESMC_ERR_INVALID_ARGUMENT;      // row points to maximise for and no column to maximise over
  if (D > kArgMaxDim) return AESMC_ERR_UNSUPPORTED;
  if (R > 0x3fffffffLL || C > 0x3fffffffLL || B > 0x7fffffffLL || B * ((R + kArgRows - 1) / kArgRows) > 0x7fffffffLL)
    return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_pairwise_argmax<float>(rows, cols, scale, scale_stride, col_a, col_sub, row_add, out, arg, flags, B, R, C,
                                         D, s);
  return launch_pairwise_argmax<double>(rows, cols, scale, scale_stride, col_a, col_sub, row_add, out, arg, flags, B, R, C,
                                        D, s);
}
