// Conditional multinomial resampling (K26): the ancestors of one conditional-SMC step with ancestor sampling (particle
// Gibbs; Andrieu, Doucet & Holenstein 2010; Lindsten, Jordan & Schoen 2014) — aesmc_conditional_ancestor_index of
// include/aesmc_hip.h.  Per batch row: K - 1 multinomial ancestors for the free slots and, in the same launch, the
// ancestor of the pinned slot K - 1, drawn with K21's scores against the reference path's next state.
//
//   workgroup = one batch row, 64 .. 1024 lanes by K (a lane per particle up to 256, four per lane beyond); lanes stride
//               over the particles;
//   scores    log_w[b,:] as float64 into LDS, and (D > 0) s[j] = gaussian_scores (pairwise_gaussian.hpp, N = 1: K21's
//             function, K21's bits) against the target row staged in LDS, into a second LDS array; both maxima and NaN
//             markers by the resampling kernels' reduction (ancestor_index.hpp);
//   weights   w = exp_nonpositive(x - max) in place, and the last particle of positive weight of either array;
//   CDF       ONE lane adds an array up in place, front to back; the two arrays by lanes of two wavefronts, side by side.
//             The contract's CDF is the sequential float64 sum; a blocked or tree scan associates the additions
//             differently, and where a row's tail weights lie near the last place of the total — wide rows, u next to 1 —
//             a different association decides a different index.  K additions that wait for one another cost some tens
//             of clocks each with their LDS traffic: microseconds at the K = 8 .. 1024 particle Gibbs runs at, and at
//             K = 4096 still 87 times below the quadratic composition it replaces.
//   search    one bisection of exactly ceil(log2 K) probes per slot over C[0 .. K-2] (C[K-1], the total, can only be
//             reached by u * total == total, where the clamp gives the same answer), slot K - 1 over the second array;
//             idx = min(count, last particle of positive weight).
//
// LDS: 8 K bytes per array, two arrays when there is a transition term, and 4.4 KiB besides: 132 KiB at the cap K = 8192.
#include "ancestor_index.hpp"
#include "conditional_cdf.hpp"
#include "pairwise_gaussian.hpp"

namespace aesmc {

constexpr int kCondMaxThreads = 1024;
constexpr int kCondMaxWaves = kCondMaxThreads / kWave;
constexpr int kCondMaxDim = 256;            // D the entry accepts, as K21's
constexpr int64_t kCondMaxParticles = 8192;

template <typename T> struct ConditionalArgs {
  const T *log_w;
  const T *loc, *target, *scale;
  int64_t loc_b, loc_k, loc_d, target_b, target_d, scale_stride;
  const double *u;
  int64_t *idx;
  int32_t *flags;
  int K, D, top;      // top: the bisection's first stride, 2^(ceil(log2 K) - 1) (0: K == 1)
};

// LDS of a launch: the CDFs, then the target row, 1 / scale, the wavefronts' maxima, the totals, the wavefronts' ints
static inline size_t conditional_lds_bytes(int64_t K, int64_t D) {
  return ((size_t)K * (D > 0 ? 2 : 1) + 2 * kCondMaxDim + 2 * kCondMaxWaves + 2) * sizeof(double) +
         2 * kCondMaxWaves * sizeof(int);
}

template <typename T>
__global__ __launch_bounds__(kCondMaxThreads) void conditional_ancestor_index_kernel(const ConditionalArgs<T> a) {
  // all of the workgroup's LDS is the launch's dynamic block (the cap raised for it leaves no room for static arrays):
  // [K] free, [K] pinned (D > 0), then the fixed part — conditional_lds_bytes
  extern __shared__ __attribute__((aligned(16))) double cond_smem[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nt / kWave;
  const int K = a.K;
  const int64_t b = blockIdx.x;
  const bool pinned = a.D > 0;
  double *free_c = cond_smem, *pin_c = cond_smem + K;
  double *tgt = cond_smem + (pinned ? 2 : 1) * (size_t)K;      // [kCondMaxDim]
  double *inv = tgt + kCondMaxDim;                             // [kCondMaxDim]
  double(*wave_max)[kCondMaxWaves] = reinterpret_cast<double(*)[kCondMaxWaves]>(inv + kCondMaxDim);      // [2][waves]
  double *totals = inv + kCondMaxDim + 2 * kCondMaxWaves;      // [2]
  int(*wave_int)[kCondMaxWaves] = reinterpret_cast<int(*)[kCondMaxWaves]>(totals + 2);                   // [2][waves]
  const T *lw = a.log_w + b * K;

  if (pinned)      // the reference's next state and 1 / scale, float64 in LDS (ends with the barrier)
    stage_tile<T, 1>(a.target + b * a.target_b, 0, a.target_d, 0, 1, a.scale, a.scale_stride, a.D, tid, nt, tgt, inv);

  // ---- scores, their maxima and NaN markers ------------------------------------------------------------------------
  double m_free = -__builtin_huge_val(), m_pin = -__builtin_huge_val();
  int nan_free = 0, nan_pin = 0;
  for (int k = tid; k < K; k += nt) {
    const double x = (double)lw[k];
    nan_free |= (x != x);
    m_free = fmax(m_free, x);      // (fmax drops a NaN operand: the marker keeps it)
    free_c[k] = x;
    if (pinned) {
      double s[1];
      gaussian_scores<T, 1>(a.loc + b * a.loc_b + (int64_t)k * a.loc_k, a.loc_d, tgt, 1, inv, a.D, x, s);
      nan_pin |= (s[0] != s[0]);
      m_pin = fmax(m_pin, s[0]);
      pin_c[k] = s[0];
    }
  }
  wave_max_nan<double>(m_free, nan_free);
  wave_max_nan<double>(m_pin, nan_pin);
  if (lane == 0) {
    wave_max[0][wave] = m_free, wave_int[0][wave] = nan_free;
    wave_max[1][wave] = m_pin, wave_int[1][wave] = nan_pin;
  }
  __syncthreads();
  const RowMax top_free = collect_max_nan(wave_max[0], wave_int[0], nwaves);
  const RowMax top_pin = collect_max_nan(wave_max[1], wave_int[1], nwaves);
  const bool bad_free = top_free.has_nan || !(fabs(top_free.dm) < __builtin_huge_val());
  const bool bad_pin = pinned && (top_pin.has_nan || !(fabs(top_pin.dm) < __builtin_huge_val()));
  if (tid == 0) {
    if (bad_free) raise_flag(a.flags, top_free.has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
    if (bad_pin) raise_flag(a.flags, top_pin.has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
  }
  int64_t *out = a.idx + b * K;
  if (bad_free) {      // (workgroup-uniform) every slot of the row, the pinned one included
    for (int k = tid; k < K; k += nt) out[k] = K;
    return;
  }
  const bool scan_pin = pinned && !bad_pin;

  // ---- weights in place, and the last particle of positive weight ----------------------------------------------------
  int last_free = -1, last_pin = -1;
  for (int k = tid; k < K; k += nt) {      // (every lane rereads what it wrote)
    const double w = exp_nonpositive(free_c[k] - top_free.dm);
    free_c[k] = w;
    if (w > 0.0) last_free = k;
    if (scan_pin) {
      const double v = exp_nonpositive(pin_c[k] - top_pin.dm);
      pin_c[k] = v;
      if (v > 0.0) last_pin = k;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    last_free = max(last_free, __shfl_xor(last_free, off, kWave));
    last_pin = max(last_pin, __shfl_xor(last_pin, off, kWave));
  }
  __syncthreads();      // the maxima's slots were read by every lane; the weights are complete
  if (lane == 0) wave_int[0][wave] = last_free, wave_int[1][wave] = last_pin;

  // ---- the CDFs: front to back, one lane each — in two wavefronts, side by side, when the workgroup has two --------------
  const int pin_lane = nt > kWave ? kWave : 0;
  if (tid == 0) totals[0] = running_sum_in_place(free_c, K);
  if (scan_pin && tid == pin_lane) totals[1] = running_sum_in_place(pin_c, K);
  __syncthreads();
  for (int w = 0; w < nwaves; ++w) {
    last_free = max(last_free, wave_int[0][w]);
    last_pin = max(last_pin, wave_int[1][w]);
  }

  // ---- one bisection per slot -------------------------------------------------------------------------------------------
  const double *u = a.u + b * K;
  for (int k = tid; k < K; k += nt) {
    int64_t drawn;
    if (k < K - 1) {
      drawn = min(count_not_above(free_c, K - 1, u[k] * totals[0], a.top), last_free);
    } else if (!pinned) {
      drawn = K - 1;
    } else if (bad_pin) {
      drawn = K;
    } else {
      drawn = min(count_not_above(pin_c, K - 1, u[k] * totals[1], a.top), last_pin);
    }
    out[k] = drawn;
  }
}

template <typename T>
static int launch_conditional_ancestor_index(const void *log_w, const double *u, const aesmc_view3 *loc,
                                             const aesmc_view3 *target, const void *scale, int64_t scale_stride,
                                             int64_t *out_idx, int32_t *flags, int64_t B, int64_t K, int64_t D,
                                             hipStream_t s) {
  ConditionalArgs<T> a = {};
  a.log_w = (const T *)log_w;
  if (D > 0) {
    a.loc = (const T *)loc->ptr;
    a.loc_b = loc->stride_b, a.loc_k = loc->stride_k, a.loc_d = loc->stride_d;
    a.target = (const T *)target->ptr;
    a.target_b = target->stride_b, a.target_d = target->stride_d;
    a.scale = (const T *)scale;
    a.scale_stride = scale_stride;
  }
  a.u = u;
  a.idx = out_idx;
  a.flags = flags;
  a.K = (int)K, a.D = (int)D;
  a.top = bisection_top(K);
  // a lane per particle up to 256 lanes, then four particles per lane up to 1024 lanes (the scores are latency-bound
  // reads of `loc`: a long row wants the wavefronts in flight)
  int64_t want = K <= 256 ? K : (K / 4 > 256 ? K / 4 : 256);
  int nt = (int)((want + kWave - 1) / kWave) * kWave;
  if (nt > kCondMaxThreads) nt = kCondMaxThreads;
  const size_t lds = conditional_lds_bytes(K, D);
  const int raised = raise_dynamic_lds_cap<conditional_ancestor_index_kernel<T>>();
  if (raised != AESMC_OK) return raised;
  hipLaunchKernelGGL((conditional_ancestor_index_kernel<T>), dim3((unsigned)B), dim3(nt), lds, s, a);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc

extern "C" int aesmc_conditional_ancestor_index(int dtype, const void *log_w, const double *u, const aesmc_view3 *loc,
                                                const aesmc_view3 *target, const void *scale, int64_t scale_stride,
                                                int64_t *out_idx, int32_t *flags, int64_t B, int64_t K, int64_t D,
                                                void *stream) {
  using namespace aesmc;
  if (log_w == nullptr || u == nullptr || out_idx == nullptr || B < 0 || K < 0 || D < 0 || (((uintptr_t)u) & 7u) != 0 ||
      (((uintptr_t)out_idx) & 7u) != 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (D > 0 && (loc == nullptr || target == nullptr || scale == nullptr || loc->ptr == nullptr ||
                target->ptr == nullptr || (scale_stride != 0 && scale_stride != 1)))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (D > kCondMaxDim || K > kCondMaxParticles || B > 0x7fffffffLL) return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_conditional_ancestor_index<float>(log_w, u, loc, target, scale, scale_stride, out_idx, flags, B, K, D, s);
  return launch_conditional_ancestor_index<double>(log_w, u, loc, target, scale, scale_stride, out_idx, flags, B, K, D, s);
}
