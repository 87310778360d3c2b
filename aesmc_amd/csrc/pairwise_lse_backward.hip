// Pairwise Gaussian weighted pass — aesmc_pairwise_pass of include/aesmc_hip.h (K25): the backward of the pairwise
// log-sum-exp (K22, pairwise_lse.hip), and with it of the marginal particle filter's log-weights.  For every batch row b
// and OWN point n, over the OTHERS m of that batch row
//
//   w[n,m]      = exp( own_term[b,n] + other_term[b,m] - 1/2 sum_d ((own[b,n,d] - others[b,m,d]) / scale[d])^2 )
//                 * own_gain[b,n] * other_gain[b,m]
//   mass[b,n]     = sum_m w[n,m]
//   pull[b,n,d]   = sum_m w[n,m] (others[b,m,d] - own[b,n,d]) / scale[d]^2
//   spread[b,n,d] = sum_m w[n,m] ((own[b,n,d] - others[b,m,d]) / scale[d])^2
//
// O(B N M D) and nothing of size [N,M] stored.  K22's backward is two launches (aesmc_amd/_ops.py: pairwise_lse): the row
// points own the columns (own_term = row_add - out, the normaliser the forward has already formed: no reference value, no
// rescale — every exponent of a finite own point is <= about 0), then the columns own the row points.
//
// The arrangement is K22's:
//   workgroup = (batch row b, tile of kRows own points), ONE wavefront; the tile's vectors and the reciprocal scales sit
//               in LDS as float64 (stage_tile: every lane reads the same address, a broadcast);
//   lanes     = others, 64 at a time: `other_term` / `other_gain` are read coalesced; the exponent is K22's score chain
//               (gaussian_scores of pairwise_gaussian.hpp) plus own_term, the weight K2's exp_nonpositive;
//   sums      every lane keeps kRows x kDims running sums of pull (and of spread) in registers, formed from the
//               DIFFERENCES (own - other) * inv — no raw moments, so nothing cancels when both clouds sit far from the
//               origin.  D above kDims = 16 goes in chunks of 16 dimensions, the weights formed again for each chunk
//               (K23's vector forms do the same with a wide payload);
//   merge     the lanes' kRows * kDims (* 2) = 64 sums are added by a HALVING butterfly: at the step over lane bit k a
//               lane keeps one half of its values and hands the other half to its partner, 63 shuffles for 64 values
//               where a full butterfly per value takes 384; lane l ends up with the total of value l and stores it.
//               Every output element has one owner: no atomics, no workspace.
// Two instantiations: pull alone with tiles of 4 own points, pull and spread with tiles of 2 (64 float64 running sums per
// lane either way); a launch that wants `mass` alone (or has D == 0) runs the first without its vector part.
//
// An absent other (other_term == -inf) and a lane beyond M contribute a SELECTED zero: the weight is selected, and the
// coordinates the differences are formed from are replaced by zeros, so nothing the absent point holds reaches a sum.
//
// Resources (the compiler's resource report, float32 / float64 operands), no scratch, no static LDS; dynamic LDS =
// 8 D (kRows + 1) bytes (10 KiB at D = 256, kRows = 4):
//   pull alone  (kRows = 4)     220 / 204 VGPR, no AGPR    2 wavefronts per SIMD
//   with spread (kRows = 2)     198 / 191 VGPR, no AGPR    2 wavefronts per SIMD
// (54 - 89 scalar registers go to vector lanes: the per-dimension branch on d < D).  Measured beside K22 and the PyTorch
// composition's backward: tools/pairwise_pass_bench.py, figures in profiles/mpf_pairwise_pass.txt.
#include "ancestor_index.hpp"
#include "pairwise_gaussian.hpp"

namespace aesmc {

constexpr int kPassMaxDim = 256;      // D the entry accepts (K22's limit: the own tile is kRows * D float64 of LDS)
constexpr int kPassDims = 16;         // dimensions per chunk: kRows * kPassDims (* 2 with spread) = 64 sums per lane
constexpr int kPassRowsPull = 4, kPassRowsSpread = 2;

template <typename T> struct PassArgs {
  const T *own, *others, *scale;
  int64_t own_b, own_n, own_d, oth_b, oth_m, oth_d, scale_stride;
  const T *own_term, *other_term, *own_gain, *other_gain;
  T *mass, *pull, *spread;
  int32_t *flags;
  int N, M, D, tiles;
};

// 64 values per lane in, their totals over the wavefront out: v[0] of lane l holds the total of value l.  At the step
// over lane bit `off` the lanes with the bit clear keep the lower half of what they still hold and send the upper half.
__device__ __forceinline__ void wave_reduce_scatter(double (&v)[kWave], int lane) {
#pragma unroll
  for (int step = 0; step < 6; ++step) {
    const int off = (kWave / 2) >> step, half = off;
    const bool upper = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const double low = v[i], high = v[i + half];
      v[i] = (upper ? high : low) + __shfl_xor(upper ? low : high, off, kWave);
    }
  }
}

template <typename T, int kRows, bool kSpread>
__global__ __launch_bounds__(kWave) void pairwise_pass_kernel(const PassArgs<T> a) {
  extern __shared__ __align__(16) double lds[];      // D * (kRows + 1) float64, sized by the launch
  double *tile = lds, *inv = lds + a.D * kRows;      // tile: [d][j]
  static_assert(kRows * kPassDims * (kSpread ? 2 : 1) == kWave, "one merged value per lane");

  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / a.tiles;
  const int n0 = (int)(blockIdx.x % a.tiles) * kRows;

  // the tile's own points (one beyond N repeats the last one and is never written) and 1 / scale
  stage_tile<T, kRows>(a.own + b * a.own_b, a.own_n, a.own_d, n0, a.N, a.scale, a.scale_stride, a.D, lane, kWave, tile,
                       inv);

  double own_term[kRows], own_gain[kRows];
  bool live[kRows];      // a finite own_term: anything else is a point the forward has dealt with — zeros, no flag
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int64_t at = b * a.N + min(n0 + j, a.N - 1);
    own_term[j] = (double)a.own_term[at];
    own_gain[j] = a.own_gain != nullptr ? (double)a.own_gain[at] : 1.0;
    live[j] = own_term[j] - own_term[j] == 0.0;
  }

  const bool vectors = a.D > 0 && (a.pull != nullptr || (kSpread && a.spread != nullptr));
  const T *others = a.others + b * a.oth_b;
  const T *other_term = a.other_term + b * a.M;
  const T *other_gain = a.other_gain != nullptr ? a.other_gain + b * a.M : nullptr;

  for (int d0 = 0; d0 == 0 || (vectors && d0 < a.D); d0 += kPassDims) {
    double mass[kRows], acc[kWave];      // acc[(j * kPassDims + dd) (+ kRows * kPassDims for spread)]
    int nan_bits = 0;
#pragma unroll
    for (int j = 0; j < kRows; ++j) mass[j] = 0.0;
#pragma unroll
    for (int i = 0; i < kWave; ++i) acc[i] = 0.0;

    for (int m0 = 0; m0 < a.M; m0 += kWave) {
      const int m = min(m0 + lane, a.M - 1);      // (a lane beyond M repeats the last other and is selected out)
      const double term = (double)other_term[m];
      const double gain = other_gain != nullptr ? (double)other_gain[m] : 1.0;
      const bool present = m0 + lane < a.M && term != -__builtin_huge_val();
      const T *x = others + (int64_t)m * a.oth_m;
      double s[kRows], w[kRows];
      gaussian_scores<T, kRows>(x, a.oth_d, tile, kRows, inv, a.D, term, s);
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const double e = own_term[j] + s[j];
        // (exp_nonpositive takes the few exponents a rounded normaliser leaves above 0 as well; NaN and +inf are NaN)
        const double p = e < __builtin_huge_val() ? exp_nonpositive(e) : __builtin_nan("");
        const double wj = (present && live[j]) ? (p * own_gain[j]) * gain : 0.0;
        nan_bits |= (wj != wj) ? (1 << j) : 0;
        w[j] = wj;
        mass[j] += wj;
      }
      if (vectors) {      // (launch-uniform)
#pragma unroll
        for (int dd = 0; dd < kPassDims; ++dd) {
          const int d = d0 + dd;
          if (d < a.D) {      // (wave-uniform)
            const double l = present ? (double)x[(int64_t)d * a.oth_d] : 0.0;
            const double iv = inv[d];
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
              const double diff = (tile[d * kRows + j] - l) * iv;
              const double wd = w[j] * diff;
              acc[j * kPassDims + dd] = __builtin_fma(-wd, iv, acc[j * kPassDims + dd]);
              if constexpr (kSpread)
                acc[(kRows + j) * kPassDims + dd] = __builtin_fma(wd, diff, acc[(kRows + j) * kPassDims + dd]);
            }
          }
        }
      }
    }

    // ---- merge the lanes' sums; lane l finishes value l ------------------------------------------------------------------
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      nan_bits |= __shfl_xor(nan_bits, off, kWave);
#pragma unroll
      for (int j = 0; j < kRows; ++j) mass[j] += __shfl_xor(mass[j], off, kWave);
    }
    if (d0 == 0) {
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (lane == j && n0 + j < a.N) {
          const bool nan = ((nan_bits >> j) & 1) != 0;
          if (nan) raise_flag(a.flags, AESMC_FLAG_NAN_LOG_WEIGHT);
          if (a.mass != nullptr) a.mass[b * a.N + n0 + j] = (T)(nan ? __builtin_nan("") : live[j] ? mass[j] : 0.0);
        }
      }
    }
    if (vectors) {
      wave_reduce_scatter(acc, lane);
      const int which = lane / (kRows * kPassDims);      // 0: pull, 1: spread
      const int j = (lane / kPassDims) % kRows, d = d0 + lane % kPassDims;
      T *out = which == 0 ? a.pull : a.spread;
      if (out != nullptr && n0 + j < a.N && d < a.D) {
        bool alive = false;
#pragma unroll
        for (int i = 0; i < kRows; ++i) alive = i == j ? live[i] : alive;
        const bool nan = ((nan_bits >> j) & 1) != 0;
        out[(b * a.N + n0 + j) * a.D + d] = (T)(nan ? __builtin_nan("") : alive ? acc[0] : 0.0);
      }
    }
  }
}

template <typename T, int kRows, bool kSpread>
static int launch_pass_form(PassArgs<T> a, int64_t B, hipStream_t s) {
  a.tiles = (a.N + kRows - 1) / kRows;      // (B * tiles fits: the entry checks it for the smallest tile)
  hipLaunchKernelGGL((pairwise_pass_kernel<T, kRows, kSpread>), dim3((unsigned)(B * a.tiles)), dim3(kWave),
                     (size_t)a.D * (kRows + 1) * sizeof(double), s, a);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

template <typename T>
static int launch_pairwise_pass(const aesmc_view3 *own, const aesmc_view3 *others, const void *scale, int64_t scale_stride,
                                const void *own_term, const void *other_term, const void *own_gain, const void *other_gain,
                                void *mass, void *pull, void *spread, int32_t *flags, int64_t B, int64_t N, int64_t M,
                                int64_t D, hipStream_t s) {
  PassArgs<T> a = {};
  if (D > 0) {
    a.own = (const T *)own->ptr;
    a.own_b = own->stride_b, a.own_n = own->stride_k, a.own_d = own->stride_d;
    a.others = (const T *)others->ptr;
    a.oth_b = others->stride_b, a.oth_m = others->stride_k, a.oth_d = others->stride_d;
    a.scale = (const T *)scale;
    a.scale_stride = scale_stride;
    a.pull = (T *)pull, a.spread = (T *)spread;
  }
  a.own_term = (const T *)own_term, a.other_term = (const T *)other_term;
  a.own_gain = (const T *)own_gain, a.other_gain = (const T *)other_gain;
  a.mass = (T *)mass;
  a.flags = flags;
  a.N = (int)N, a.M = (int)M, a.D = (int)D;
  if (a.spread != nullptr) return launch_pass_form<T, kPassRowsSpread, true>(a, B, s);
  return launch_pass_form<T, kPassRowsPull, false>(a, B, s);
}

}  // namespace aesmc

extern "C" int aesmc_pairwise_pass(int dtype, const aesmc_view3 *own, const aesmc_view3 *others, const void *scale,
                                   int64_t scale_stride, const void *own_term, const void *other_term,
                                   const void *own_gain, const void *other_gain, void *mass, void *pull, void *spread,
                                   int32_t *flags, int64_t B, int64_t N, int64_t M, int64_t D, void *stream) {
  using namespace aesmc;
  if (own_term == nullptr || other_term == nullptr || B < 0 || N < 0 || M < 0 || D < 0) return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (mass == nullptr && (D == 0 || (pull == nullptr && spread == nullptr))) return AESMC_ERR_INVALID_ARGUMENT;   // no output
  if (D > 0 && (own == nullptr || others == nullptr || scale == nullptr || own->ptr == nullptr || others->ptr == nullptr ||
                (scale_stride != 0 && scale_stride != 1)))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0) return AESMC_OK;
  if (M == 0) return AESMC_ERR_INVALID_ARGUMENT;      // own points to sum for and nothing to sum over
  if (D > kPassMaxDim) return AESMC_ERR_UNSUPPORTED;
  if (N > 0x3fffffffLL || M > 0x3fffffffLL || B > 0x7fffffffLL ||
      B * ((N + kPassRowsSpread - 1) / kPassRowsSpread) > 0x7fffffffLL)
    return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_pairwise_pass<float>(own, others, scale, scale_stride, own_term, other_term, own_gain, other_gain, mass,
                                       pull, spread, flags, B, N, M, D, s);
  return launch_pairwise_pass<double>(own, others, scale, scale_stride, own_term, other_term, own_gain, other_gain, mass,
                                      pull, spread, flags, B, N, M, D, s);
}
