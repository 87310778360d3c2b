// Pairwise Gaussian softmax mean — aesmc_pairwise_mean of include/aesmc_hip.h (K23): the building block of the two-slice
// particle smoother.  For every batch row b and row point r, with s[r,c] the score K22 sums (pairwise_lse.hip)
//
//   out[b,r,p] = sum_c softmax_c(s[r,:])[c] * payload[b,c,p]          lse[b,r] = row_add[b,r] + log sum_c exp(s[r,c])
//
// attention with Gaussian scores in float64: O(B R C (D + P)) and nothing of size [R,C] stored.  `lse` is K22's result,
// bit for bit (the same scores, the same reference moves, the same sums, the same merge), so one launch of this kernel
// replaces the first of K22's two launches per backward step and returns the backward kernel's mean of a payload too.
//
// The pass is K22's: workgroup = (batch row b, tile of row points), ONE wavefront; lanes = columns, 64 at a time; one
// wave-uniform reference per row point, moved on a vote, the lanes' sums AND the payload accumulators rescaled on the move;
// exp_nonpositive for the weights; float64 throughout.  What is new is the [rows] x [64] block of weights times the
// [64] x [P] block of payload per step.  Two forms, measured beside each other (tools/pairwise_mean_bench.py, figures in
// profiles/ffbsm_pairwise_mean.txt) and walked by aesmc_test_set_pairwise_mean_form:
//
//   matrix cores (form 1)  tile of 16 row points.  The step's weights go to LDS as E[c][j] (64 x 16 float64, rows padded
//       to 17: 8.5 KiB); each of the 16 k-steps of v_mfma_f64_16x16x4_f64 takes A = E[column 4k + (l >> 4)][row l & 15]
//       from LDS and B = payload[column 4k + (l >> 4)][p0 + (l & 15)] from memory, converted to double; one accumulator
//       quad per 16 payload values (kQuads = 1, 2, 4, 8, 16 for P <= 16 .. 256), result (row, p) = ((l >> 4) + 4 * reg,
//       l & 15) — the float64 map, not the float32 one.  A quad is rescaled by its rows' factors when a reference moves.
//   vector pipe (forms 2, 3)  lanes stay columns, every lane holds kRows x kP = 4 x 16 (2 x 32) float64 accumulators, merged
//       by the shuffle tree at the end; payload wider than kP goes in chunks, the scores formed again for each.
//
// An absent column (col_a == -inf) and a lane beyond C contribute a SELECTED zero, never 0 * payload.
//
// Measured at B = 64, R = C = 1024, D = 10, float32 (one MI355X): the matrix cores 463 us at P = 10 and 858 us at P = 64, the
// vector pipe 1126 / 4511 us (4 x 16) and 2677 / 6002 us (2 x 32); K22 on the same operands 221 us; the PyTorch float64
// composition 8967 / 8999 us.  The library launches the matrix-core form; the vector forms stay as measurement forms.
//
// Resources of the launched form (the compiler's resource report, float32 / float64 operands): LDS = 9040 bytes static
// (the weights 8704, the finishing slots) + 136 D bytes for the tile and the reciprocal scales, no scratch;
//   P <= 16    160 / 161 VGPR +   8 AGPR    3 / 2 wavefronts per SIMD        P <= 128   235 VGPR +  64 AGPR    1 per SIMD
//   P <= 32    172 VGPR       +  16 AGPR    2 per SIMD                       P <= 256   256 VGPR + 252 AGPR    1 per SIMD
//   P <= 64    194 VGPR       +  32 AGPR    2 per SIMD
// At D = 256, P = 256 the LDS is 34 KiB for the tile + 8.8 KiB = 43 KiB per workgroup: three workgroups per CU by LDS, but
// the 508 registers leave one wavefront per SIMD; at D = 10, P = 10 (10.4 KiB, 168 registers) the registers decide: 3.
#include "ancestor_index.hpp"
#include "pairwise_gaussian.hpp"

namespace aesmc {

constexpr int kMeanMaxDim = 256;          // D: the row tile is 16 * D float64 of LDS
constexpr int kMeanMaxPayload = 256;      // P: 16 accumulator quads of the matrix-core form
constexpr int kMeanTile = 16;             // row points per workgroup of the matrix-core form
constexpr int kMeanPad = kMeanTile + 1;   // E[c][j]: lane c writes 16 values at c * 17 (no two lanes of a half on one bank)

typedef double mean_quad __attribute__((ext_vector_type(4)));

template <typename T> struct PairwiseMeanArgs {
  PairwiseArgs<T> s;      // the scores' operands; s.out is lse_out (may be NULL)
  const T *payload;
  int64_t pay_b, pay_c, pay_p;
  T *mean;                // [B,R,P] dense
  int P;
};

// what a finished row point is: K22's rules, applied by whoever finishes it
enum { kMeanFinite = 0, kMeanNan = 1, kMeanDegenerate = 2, kMeanEmpty = 3 };

// the row point's lse (K22's finishing formula) and its kind from (reference, sum, NaN seen, row_add)
__device__ __forceinline__ int finish_row_point(double top, double total, bool nan, double add, double &value) {
  if (nan || add != add) {
    value = __builtin_nan("");
    return kMeanNan;
  }
  if (top == __builtin_huge_val()) {
    value = top;
    return kMeanDegenerate;
  }
  if (top == -__builtin_huge_val()) {
    value = top;      // every score -inf: a point of zero weight, no flag
    return kMeanEmpty;
  }
  value = add + (top + ::log(total));
  return kMeanFinite;
}

__device__ __forceinline__ void raise_for_kind(int32_t *flags, int kind) {
  if (kind == kMeanNan) raise_flag(flags, AESMC_FLAG_NAN_LOG_WEIGHT);
  if (kind == kMeanDegenerate) raise_flag(flags, AESMC_FLAG_DEGENERATE_ROW);
}

// out[b,r,p] of a finished row point from its accumulator
__device__ __forceinline__ double mean_value(int kind, double acc, double total) {
  if (kind == kMeanFinite) return acc / total;
  return kind == kMeanEmpty ? 0.0 : __builtin_nan("");
}

// ---- form 1: the payload product on the float64 matrix cores ----------------------------------------------------------------
template <typename T, int kQuads>
__global__ __launch_bounds__(kWave) void pairwise_mean_mfma_kernel(const PairwiseMeanArgs<T> m) {
  constexpr int kRows = kMeanTile;
  extern __shared__ __align__(16) double lds[];      // D * (kRows + 1) float64, sized by the launch
  __shared__ double weights[kWave * kMeanPad];       // E[c][j] of the step
  __shared__ double fin_ref[kRows], fin_sum[kRows];
  __shared__ int fin_kind[kRows];
  __shared__ int fin_nan;
  const PairwiseArgs<T> &a = m.s;
  double *tile = lds, *inv = lds + a.D * kRows;      // tile: [d][j]

  const int lane = threadIdx.x;
  const int group = lane >> 4, n = lane & 15;        // the lane's place in an MFMA operand: k (or row) group, row (or p)
  const int64_t b = blockIdx.x / a.tiles;
  const int r0 = (int)(blockIdx.x % a.tiles) * kRows;

  stage_tile<T, kRows>(a.rows + b * a.rows_b, a.rows_r, a.rows_d, r0, a.R, a.scale, a.scale_stride, a.D, lane, kWave,
                       tile, inv);

  double ref[kRows], sum[kRows];      // ref: the same in every lane
  mean_quad acc[kQuads];              // acc[q][reg]: row point (group + 4 * reg), payload value 16 q + n
  int nan_bits = 0;
#pragma unroll
  for (int j = 0; j < kRows; ++j) ref[j] = -__builtin_huge_val(), sum[j] = 0.0;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) acc[q] = (mean_quad){0.0, 0.0, 0.0, 0.0};

  const T *col_a = a.col_a + b * a.C;
  const T *payload = m.payload + b * m.pay_b;
  for (int c0 = 0; c0 < a.C; c0 += kWave) {
    const int c = c0 + lane;
    double s[kRows], factor[kRows];
    bool moved = false;
    pairwise_scores<T, kRows>(a, tile, inv, b, min(c, a.C - 1), s);
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const double sj = c < a.C ? s[j] : -__builtin_huge_val();
      nan_bits |= (sj != sj) ? (1 << j) : 0;
      factor[j] = 1.0;
      if (__ballot(sj > ref[j]) != 0) {      // (wave-uniform)  some lane's score is above the reference
        const double top = wave_max_uniform(sj);
        factor[j] = exp_nonpositive(ref[j] - top);      // (from -inf: the sums are still zero and stay so)
        sum[j] *= factor[j];
        ref[j] = top;
        moved = true;
      }
      const double e = exp_nonpositive(sj - ref[j]);    // (NaN and -inf - -inf give 0: see exp_nonpositive's guard)
      sum[j] += e;
      weights[lane * kMeanPad + j] = e;
    }
    if (moved) {      // (wave-uniform)  the accumulators follow their rows' references
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const double f = group == 0 ? factor[4 * reg] : group == 1 ? factor[4 * reg + 1] : group == 2 ? factor[4 * reg + 2]
                                                                                                       : factor[4 * reg + 3];
#pragma unroll
        for (int q = 0; q < kQuads; ++q) acc[q][reg] *= f;
      }
    }
    __syncthreads();
    const int steps = min(16, (a.C - c0 + 3) >> 2);      // k-steps that hold a column below C
    for (int k = 0; k < steps; ++k) {
      const int cc = c0 + 4 * k + group, held = min(cc, a.C - 1);
      const double e = weights[(4 * k + group) * kMeanPad + n];
      const bool present = cc < a.C && (double)col_a[held] != -__builtin_huge_val();
      const T *from = payload + (int64_t)held * m.pay_c;
#pragma unroll
      for (int q = 0; q < kQuads; ++q) {
        const int p = 16 * q + n;
        const double v = (double)from[(int64_t)min(p, m.P - 1) * m.pay_p];
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(e, (present && p < m.P) ? v : 0.0, acc[q], 0, 0, 0);
      }
    }
    __syncthreads();      // (the next step writes the weights again)
  }

  // ---- the lanes' sums are added up; lane j finishes row point r0 + j, then every lane writes its accumulators -----------
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    nan_bits |= __shfl_xor(nan_bits, off, kWave);
#pragma unroll
    for (int j = 0; j < kRows; ++j) sum[j] += __shfl_xor(sum[j], off, kWave);
  }
  if (lane == 0) {
    fin_nan = nan_bits;
#pragma unroll
    for (int j = 0; j < kRows; ++j) fin_ref[j] = ref[j], fin_sum[j] = sum[j];
  }
  __syncthreads();
  if (lane < kRows) {
    const int j = lane;
    int kind = kMeanEmpty;
    if (r0 + j < a.R) {
      const int64_t at = b * a.R + r0 + j;
      const double add = a.row_add != nullptr ? (double)a.row_add[at] : 0.0;
      double value;
      kind = finish_row_point(fin_ref[j], fin_sum[j], (fin_nan >> j) & 1, add, value);
      raise_for_kind(a.flags, kind);
      if (a.out != nullptr) a.out[at] = (T)value;
    }
    fin_kind[j] = kind;
  }
  __syncthreads();
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int j = group + 4 * reg;
    if (r0 + j >= a.R) continue;
    const int kind = fin_kind[j];
    const double total = fin_sum[j];
    T *to = m.mean + (b * a.R + r0 + j) * m.P;
#pragma unroll
    for (int q = 0; q < kQuads; ++q) {
      const int p = 16 * q + n;
      if (p < m.P) to[p] = (T)mean_value(kind, acc[q][reg], total);
    }
  }
}

// ---- forms 2, 3: the payload product on the vector pipe, kRows x kP accumulators in every lane -------------------------------
template <typename T, int kRows, int kP>
__global__ __launch_bounds__(kWave) void pairwise_mean_vector_kernel(const PairwiseMeanArgs<T> m) {
  static_assert(kRows * kP == kWave, "one finishing lane per (row point, payload value) of a chunk");
  extern __shared__ __align__(16) double lds[];      // D * (kRows + 1) float64, sized by the launch
  __shared__ double fin_acc[kWave];
  __shared__ double fin_ref[kRows], fin_sum[kRows];
  __shared__ int fin_nan;
  const PairwiseArgs<T> &a = m.s;
  double *tile = lds, *inv = lds + a.D * kRows;

  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / a.tiles;
  const int r0 = (int)(blockIdx.x % a.tiles) * kRows;

  stage_tile<T, kRows>(a.rows + b * a.rows_b, a.rows_r, a.rows_d, r0, a.R, a.scale, a.scale_stride, a.D, lane, kWave,
                       tile, inv);

  const T *col_a = a.col_a + b * a.C;
  const T *payload = m.payload + b * m.pay_b;
  for (int p0 = 0; p0 < m.P; p0 += kP) {      // payload wider than kP: one whole pass per chunk, the scores formed again
    double ref[kRows], sum[kRows], acc[kRows][kP];
    int nan_bits = 0;
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      ref[j] = -__builtin_huge_val(), sum[j] = 0.0;
#pragma unroll
      for (int p = 0; p < kP; ++p) acc[j][p] = 0.0;
    }
    for (int c0 = 0; c0 < a.C; c0 += kWave) {
      const int c = c0 + lane, held = min(c, a.C - 1);
      double s[kRows], v[kP];
      pairwise_scores<T, kRows>(a, tile, inv, b, held, s);
      const bool present = c < a.C && (double)col_a[held] != -__builtin_huge_val();
      const T *from = payload + (int64_t)held * m.pay_c;
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        const double loaded = (double)from[(int64_t)min(p0 + p, m.P - 1) * m.pay_p];
        v[p] = (present && p0 + p < m.P) ? loaded : 0.0;
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const double sj = c < a.C ? s[j] : -__builtin_huge_val();
        nan_bits |= (sj != sj) ? (1 << j) : 0;
        if (__ballot(sj > ref[j]) != 0) {      // (wave-uniform)
          const double top = wave_max_uniform(sj);
          const double f = exp_nonpositive(ref[j] - top);
          sum[j] *= f;
#pragma unroll
          for (int p = 0; p < kP; ++p) acc[j][p] *= f;
          ref[j] = top;
        }
        const double e = exp_nonpositive(sj - ref[j]);
        sum[j] += e;
#pragma unroll
        for (int p = 0; p < kP; ++p) acc[j][p] = __builtin_fma(e, v[p], acc[j][p]);
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      nan_bits |= __shfl_xor(nan_bits, off, kWave);
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        sum[j] += __shfl_xor(sum[j], off, kWave);
#pragma unroll
        for (int p = 0; p < kP; ++p) acc[j][p] += __shfl_xor(acc[j][p], off, kWave);
      }
    }
    if (lane == 0) {
      fin_nan = nan_bits;
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        fin_ref[j] = ref[j], fin_sum[j] = sum[j];
#pragma unroll
        for (int p = 0; p < kP; ++p) fin_acc[j * kP + p] = acc[j][p];
      }
    }
    __syncthreads();
    {      // lane j * kP + p finishes payload value p0 + p of row point r0 + j; the first of a row point also its lse
      const int j = lane / kP, p = lane % kP;
      if (r0 + j < a.R) {
        const int64_t at = b * a.R + r0 + j;
        const double add = a.row_add != nullptr ? (double)a.row_add[at] : 0.0;
        double value;
        const int kind = finish_row_point(fin_ref[j], fin_sum[j], (fin_nan >> j) & 1, add, value);
        if (p == 0 && p0 == 0) {
          raise_for_kind(a.flags, kind);
          if (a.out != nullptr) a.out[at] = (T)value;
        }
        if (p0 + p < m.P) m.mean[at * m.P + p0 + p] = (T)mean_value(kind, fin_acc[lane], fin_sum[j]);
      }
    }
    __syncthreads();      // (the next chunk writes fin_* again)
  }
}

// which form a launch takes: 0 = the default; tools/pairwise_mean_bench.py walks the others through the test hook
static int g_mean_form = 0;
constexpr int kMeanDefaultForm = 1;

template <typename T, int kQuads> static int launch_mean_mfma(PairwiseMeanArgs<T> m, int64_t B, hipStream_t s) {
  m.s.tiles = (m.s.R + kMeanTile - 1) / kMeanTile;
  hipLaunchKernelGGL((pairwise_mean_mfma_kernel<T, kQuads>), dim3((unsigned)(B * m.s.tiles)), dim3(kWave),
                     (size_t)m.s.D * (kMeanTile + 1) * sizeof(double), s, m);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

template <typename T, int kRows, int kP> static int launch_mean_vector(PairwiseMeanArgs<T> m, int64_t B, hipStream_t s) {
  m.s.tiles = (m.s.R + kRows - 1) / kRows;      // (B * tiles fits: the entry checks it for the smallest tile)
  hipLaunchKernelGGL((pairwise_mean_vector_kernel<T, kRows, kP>), dim3((unsigned)(B * m.s.tiles)), dim3(kWave),
                     (size_t)m.s.D * (kRows + 1) * sizeof(double), s, m);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

template <typename T>
static int launch_pairwise_mean(const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale, int64_t scale_stride,
                                const void *col_a, const void *col_sub, const void *row_add, const aesmc_view3 *payload,
                                void *out, void *lse_out, int32_t *flags, int64_t B, int64_t R, int64_t C, int64_t D,
                                int64_t P, hipStream_t s) {
  PairwiseMeanArgs<T> m = {};
  PairwiseArgs<T> &a = m.s;
  if (D > 0) {
    a.rows = (const T *)rows->ptr;
    a.rows_b = rows->stride_b, a.rows_r = rows->stride_k, a.rows_d = rows->stride_d;
    a.cols = (const T *)cols->ptr;
    a.cols_b = cols->stride_b, a.cols_c = cols->stride_k, a.cols_d = cols->stride_d;
    a.scale = (const T *)scale;
    a.scale_stride = scale_stride;
  }
  a.col_a = (const T *)col_a, a.col_sub = (const T *)col_sub, a.row_add = (const T *)row_add;
  a.out = (T *)lse_out;
  a.flags = flags;
  a.R = (int)R, a.C = (int)C, a.D = (int)D;
  m.payload = (const T *)payload->ptr;
  m.pay_b = payload->stride_b, m.pay_c = payload->stride_k, m.pay_p = payload->stride_d;
  m.mean = (T *)out;
  m.P = (int)P;
  switch (g_mean_form ? g_mean_form : kMeanDefaultForm) {
    case 1:
      if (P <= 16) return launch_mean_mfma<T, 1>(m, B, s);
      if (P <= 32) return launch_mean_mfma<T, 2>(m, B, s);
      if (P <= 64) return launch_mean_mfma<T, 4>(m, B, s);
      if (P <= 128) return launch_mean_mfma<T, 8>(m, B, s);
      return launch_mean_mfma<T, 16>(m, B, s);
    case 2:
      return launch_mean_vector<T, 4, 16>(m, B, s);
    case 3:
      return launch_mean_vector<T, 2, 32>(m, B, s);
  }
  return AESMC_ERR_INVALID_ARGUMENT;
}

}  // namespace aesmc

extern "C" int aesmc_pairwise_mean(int dtype, const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale,
                                   int64_t scale_stride, const void *col_a, const void *col_sub, const void *row_add,
                                   const aesmc_view3 *payload, void *out, void *lse_out, int32_t *flags, int64_t B,
                                   int64_t R, int64_t C, int64_t D, int64_t P, void *stream) {
  using namespace aesmc;
  if (col_a == nullptr || out == nullptr || payload == nullptr || payload->ptr == nullptr || B < 0 || R < 0 || C < 0 ||
      D < 0 || P < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (D > 0 && (rows == nullptr || cols == nullptr || scale == nullptr || rows->ptr == nullptr || cols->ptr == nullptr ||
                (scale_stride != 0 && scale_stride != 1)))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || R == 0) return AESMC_OK;
  if (C == 0) return AESMC_ERR_INVALID_ARGUMENT;      // row points to average for and no column to average over
  if (D > kMeanMaxDim || P > kMeanMaxPayload) return AESMC_ERR_UNSUPPORTED;
  if (R > 0x3fffffffLL || C > 0x3fffffffLL || B > 0x7fffffffLL || B * ((R + 1) / 2) > 0x7fffffffLL)
    return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_pairwise_mean<float>(rows, cols, scale, scale_stride, col_a, col_sub, row_add, payload, out, lse_out,
                                       flags, B, R, C, D, P, s);
  return launch_pairwise_mean<double>(rows, cols, scale, scale_stride, col_a, col_sub, row_add, payload, out, lse_out,
                                      flags, B, R, C, D, P, s);
}

// Measurement / test hook (not part of include/aesmc_hip.h): the form of the launches that follow — 0 the default, 1 the
// matrix cores, 2 / 3 the vector pipe with 4 x 16 / 2 x 32 accumulators per lane.
extern "C" int aesmc_test_set_pairwise_mean_form(int form) {
  if (form < 0 || form > 3) return AESMC_ERR_INVALID_ARGUMENT;
  aesmc::g_mean_form = form;
  return AESMC_OK;
}
