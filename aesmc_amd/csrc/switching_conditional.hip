// Conditional multinomial resampling for the regimes of a switching linear-Gaussian model (K37): the ancestors of one step of
// a Rao-Blackwellised conditional particle filter with ancestor sampling (particle Gibbs on the regimes; Whiteley, Andrieu &
// Doucet 2010; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016) — aesmc_switching_conditional_ancestor_index of
// include/aesmc_hip.h.  K26 (conditional_ancestor_index.hip) with the pinned slot's Gaussian-transition score replaced by
// K35's closed-form integral (switching_score.hpp) against the ONE reference trajectory of the batch row: with z integrated
// out the regimes are not Markov, and what the reference's future says about a stored particle (s, m, P) is K34's (F, lam).
//
//   workgroup = one batch row; 64 lanes up to K = 64, 256 beyond; lanes stride over the particles;
//   staged    the row's F, lam (zero-padded to the instantiation's extent DP = 2, 4, 8) and the column log Pi[., s'] into LDS
//             once, read as broadcasts (the column at the lane's regime: distinct banks);
//   scores    log_w[b,:] into the first LDS array and s[j] = switching_pair_score (K35's function, K35's bits) into the
//             second; both maxima and NaN markers by the resampling kernels' reduction (ancestor_index.hpp);
//   P         DP = 2, 4: the lane's packed covariance in registers; DP = 8: in LDS in K31's [element][lane] layout (SkCov,
//             consecutive lanes on consecutive 8-byte words: no conflicts), 72 KB at 256 lanes, 18 KB at 64 — the same
//             choice as K35's, whose 8-wide score is 200 registers with it;
//   weights, CDF, search   K26's, from conditional_cdf.hpp: w = exp_nonpositive(x - max) in place, ONE lane adds an array up
//             front to back (the two arrays by lanes of two wavefronts, side by side, when the workgroup has two), one
//             bisection of exactly ceil(log2 K) probes per slot, idx = min(count, last particle of positive weight).
//
// LDS: 8 K bytes per array (two with ancestor sampling), the covariances at DP = 8, and (TP + DP + 16 + 14) float64 besides.
// The cap is 8192 particles up to D = 4 (128 KB + 0.4 KB) and 4096 above (64 KB + 72 KB + 0.6 KB), inside the 160 KB of a
// compute unit: aesmc_switching_conditional_max_particles(D).
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950):
//   <DP,lanes>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2,64>         76      0        0             6
//   <2,256>        76      0        0             6
//   <4,64>        150      0        0             3
//   <4,256>       150      0        0             3
//   <8,64>        229      0        0             2       P in LDS (18 KB)
//   <8,256>       233      0        0             2       P in LDS (72 KB)
// No instantiation spills.  Measured (profiles/switching_gibbs.txt, B = 1024): 15 us at K = 64, D = 4 and 351 us at K = 1024,
// D = 8, against 43 us and 327 us for the four launches it replaces.
#include "ancestor_index.hpp"
#include "conditional_cdf.hpp"
#include "switching_host.hpp"
#include "switching_score.hpp"

namespace aesmc {

constexpr int kScMaxWaves = 4;      // 256 lanes

static inline int64_t sc_max_particles(int64_t D) { return D <= 4 ? 8192 : 4096; }

struct SwitchingConditionalArgs {
  const double *log_w, *u;          // [B,K]
  const double *log_Pi;             // [M,M]
  const int32_t *regime_next;       // [B]
  const double *factor, *lambda;    // [B,D(D+1)/2], [B,D]; both NULL: no ancestor sampling
  const int32_t *regime;            // [B,K]
  const double *mean, *cov;         // [B,K,D], [B,K,D(D+1)/2]
  int64_t *idx;                     // [B,K]
  int32_t *flags;
  int K, M, D, top;                 // top: the bisection's first stride (bisection_top)
};

// float64 words of a launch's LDS behind the CDFs: F, lam, the column of log Pi, the wavefronts' maxima, the totals, the
// wavefronts' ints; then, for DP == 8, [TP][lanes] covariances
__host__ __device__ constexpr int sc_fixed_doubles(int dp) {
  return dp * (dp + 1) / 2 + dp + kSkMaxRegimes + 2 * kScMaxWaves + 2 + kScMaxWaves;
}
static inline size_t sc_lds_bytes(int64_t K, int dp, int lanes, bool pinned) {
  return ((size_t)K * (pinned ? 2 : 1) + sc_fixed_doubles(dp) +
          (pinned && sk_cov_in_lds(dp) ? (size_t)dp * (dp + 1) / 2 * lanes : 0)) * sizeof(double);
}

template <int DP, int NT>
__global__ __launch_bounds__(NT) void switching_conditional_kernel(const SwitchingConditionalArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sc_smem[];
  constexpr int TP = DP * (DP + 1) / 2;
  constexpr int nwaves = NT / kWave;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int K = a.K, M = a.M, D = a.D;
  const int TD = D * (D + 1) / 2;
  const int64_t b = blockIdx.x;
  const bool pinned = a.factor != nullptr;
  double *free_c = sc_smem, *pin_c = sc_smem + K;
  double *Ft = sc_smem + (pinned ? 2 : 1) * (size_t)K;      // [TP]
  double *lt = Ft + TP;                                     // [DP]
  double *pt = lt + DP;                                     // [kSkMaxRegimes]: log Pi[s, s'] by s
  double(*wave_max)[kScMaxWaves] = reinterpret_cast<double(*)[kScMaxWaves]>(pt + kSkMaxRegimes);      // [2][waves]
  double *totals = pt + kSkMaxRegimes + 2 * kScMaxWaves;    // [2]
  int(*wave_int)[kScMaxWaves] = reinterpret_cast<int(*)[kScMaxWaves]>(totals + 2);                    // [2][waves]
  const double *lw = a.log_w + b * K;

  if (pinned) {      // the reference's (F, lam) and its column of log Pi, float64 in LDS
    for (int e = tid; e < TP; e += NT) Ft[e] = e < TD ? a.factor[b * TD + e] : 0.0;
    for (int e = tid; e < DP; e += NT) lt[e] = e < D ? a.lambda[b * D + e] : 0.0;
    const int next = a.regime_next[b];
    const bool outside = next < 0 || next >= M;      // (a NaN column: every score of the row is NaN)
    if (outside && tid == 0) raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    for (int s = tid; s < M; s += NT) pt[s] = outside ? Num<double>::nan() : a.log_Pi[s * M + next];
    __syncthreads();
  }

  // ---- scores, their maxima and NaN markers ------------------------------------------------------------------------
  double m_free = -__builtin_huge_val(), m_pin = -__builtin_huge_val();
  int nan_free = 0, nan_pin = 0;
  for (int k = tid; k < K; k += NT) {
    const double x = lw[k];
    nan_free |= (x != x);
    m_free = fmax(m_free, x);      // (fmax drops a NaN operand: the marker keeps it)
    free_c[k] = x;
    if (pinned) {
      const int64_t particle = b * K + k;
      const int s = a.regime[particle];
      double score;
      if (s < 0 || s >= M) {
        raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
        score = Num<double>::nan();
      } else {
        double m[DP];
        SkCov<TP, sk_cov_in_lds(DP), NT> P;
        P.lds = reinterpret_cast<double *>(wave_int + 2) + tid;
        const double *mrow = a.mean + particle * D, *prow = a.cov + particle * TD;
#pragma unroll
        for (int i = 0; i < DP; ++i) m[i] = i < D ? mrow[i] : 0.0;
#pragma unroll
        for (int e = 0; e < TP; ++e) P.set(e, e < TD ? prow[e] : 0.0);
        score = switching_pair_score<DP>(Ft, lt, m, P, pt + s, x, true);
      }
      nan_pin |= (score != score);
      m_pin = fmax(m_pin, score);
      pin_c[k] = score;
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
    for (int k = tid; k < K; k += NT) out[k] = K;
    return;
  }
  const bool scan_pin = pinned && !bad_pin;

  // ---- weights in place, and the last particle of positive weight ----------------------------------------------------
  int last_free = -1, last_pin = -1;
  for (int k = tid; k < K; k += NT) {      // (every lane rereads what it wrote)
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
  const int pin_lane = NT > kWave ? kWave : 0;
  if (tid == 0) totals[0] = running_sum_in_place(free_c, K);
  if (scan_pin && tid == pin_lane) totals[1] = running_sum_in_place(pin_c, K);
  __syncthreads();
  for (int w = 0; w < nwaves; ++w) {
    last_free = max(last_free, wave_int[0][w]);
    last_pin = max(last_pin, wave_int[1][w]);
  }

  // ---- one bisection per slot -------------------------------------------------------------------------------------------
  const double *u = a.u + b * K;
  for (int k = tid; k < K; k += NT) {
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

// (not sk_launch: this kernel's limit is raised once per device, as the resampling kernels' is)
template <int DP, int NT> static int sc_launch(int64_t B, size_t lds, hipStream_t s, const SwitchingConditionalArgs &a) {
  const int raised = raise_dynamic_lds_cap<switching_conditional_kernel<DP, NT>>();
  if (raised != AESMC_OK) return raised;
  hipLaunchKernelGGL((switching_conditional_kernel<DP, NT>), dim3((unsigned)B), dim3(NT), lds, s, a);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc

extern "C" int64_t aesmc_switching_conditional_max_particles(int64_t D) {
  return D < 1 || D > aesmc::kSkMaxDim ? 0 : aesmc::sc_max_particles(D);
}

extern "C" int aesmc_switching_conditional_ancestor_index(const double *log_w, const double *u, const double *log_Pi,
                                                          const int32_t *regime_next, const double *factor,
                                                          const double *lambda, const int32_t *regime, const double *mean,
                                                          const double *cov, int64_t *out_idx, int32_t *flags, int64_t B,
                                                          int64_t K, int64_t M, int64_t D, void *stream) {
  using namespace aesmc;
  if (log_w == nullptr || u == nullptr || out_idx == nullptr || B < 0 || K < 0 || !sk_extents_positive(M, D, 1))
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool pinned = factor != nullptr;
  if (pinned != (lambda != nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (pinned && (log_Pi == nullptr || regime_next == nullptr || regime == nullptr || mean == nullptr || cov == nullptr))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(log_w, 8) || !sk_aligned(u, 8) || !sk_aligned(log_Pi, 8) || !sk_aligned(regime_next, 4) ||
      !sk_aligned(factor, 8) || !sk_aligned(lambda, 8) || !sk_aligned(regime, 4) || !sk_aligned(mean, 8) ||
      !sk_aligned(cov, 8) || !sk_aligned(out_idx, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({out_idx}, {log_w, u, log_Pi, regime_next, factor, lambda, regime, mean, cov}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (!sk_extents_supported(M, D, 1) || K > sc_max_particles(D) || !sk_fits_32bit(B, K, kSkTriMax)) return AESMC_ERR_UNSUPPORTED;
  SwitchingConditionalArgs a;
  a.log_w = log_w, a.u = u, a.log_Pi = log_Pi, a.regime_next = regime_next;
  a.factor = factor, a.lambda = lambda, a.regime = regime, a.mean = mean, a.cov = cov;
  a.idx = out_idx, a.flags = flags;
  a.K = (int)K, a.M = (int)M, a.D = (int)D;
  a.top = bisection_top(K);
  const int dp = sk_pad(D);
  const int lanes = K <= kWave ? kWave : kSkBlock;
  const size_t lds = sc_lds_bytes(K, dp, lanes, pinned);
  hipStream_t s = (hipStream_t)stream;
  return sk_for_extent(dp, [&](auto d) {
    constexpr int DP = decltype(d)::value;
    return lanes == kWave ? sc_launch<DP, kWave>(B, lds, s, a) : sc_launch<DP, kSkBlock>(B, lds, s, a);
  });
}
