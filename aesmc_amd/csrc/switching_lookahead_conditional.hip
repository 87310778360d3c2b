// The resampling side of a LOOK-AHEAD conditional sweep for a switching linear-Gaussian model (K48): the look-ahead of the
// fully adapted Rao-Blackwellised filter (K32, switching_lookahead.hip) on a stored system and the conditional ancestors on
// its first-stage weights (K37, switching_conditional.hip) in ONE launch — aesmc_switching_lookahead_conditional_ancestor_index
// of include/aesmc_hip.h, and under a mask of the observation's components aesmc_switching_masked_lookahead_conditional_
// ancestor_index (K40's selections).  Particle Gibbs runs 8 .. 64 particles and is bound by its launches: composed from
// existing ones this step is K32, K37 on the first-stage weights and K37 on zeros for the pinned slot.
//
// After a look-ahead draw the K weights of a stored system are EQUAL.  So the free slots resample on the first-stage weights
// v_j = log p(y_t | history_j) alone, and the pinned slot's ancestor score is Pi[s_j, s'_t] x K35's integral with a log-weight
// of exactly 0.0: it does NOT carry v_j (the weights that enter ancestor sampling are those of system t-1).
//
//   workgroup = one batch row; 64 lanes up to K = 64, 256 beyond; lanes stride over the particles (K37's geometry);
//   staged    log Pi [M,M] and the model as K32 stages them; the row's F, lam and the column log Pi[., s'] as K37 does;
//   per particle   K32's run-time loop over the regimes with the same chains in the same order (predict, U = C P-, S, the
//             Cholesky factor, ONE solve, the score), the scores in LDS [M][lanes]; their log-sum-exp to `log_weight` and
//             into the first LDS array of K, the cumulative row to `cdf`; then, with ancestor sampling,
//             switching_pair_score (K35's function, K35's bits) with the log-weight 0.0 into the second array;
//   P         DP = 8: ONE [TP][lanes] LDS buffer is first the look-ahead's predicted covariance and then the pair score's
//             stored P (the live ranges do not overlap); DP = 2, 4: registers, as K32 and K37;
//   tail      K37's, through conditional_cdf.hpp: maxima and NaN markers, weights in place, ONE lane per running sum, one
//             bisection of exactly ceil(log2 K) probes per slot.
//
// LDS, in float64 words: (1 or 2) K for the arrays, K37's fixed words TP + DP + 16 + 14, M M for log Pi, M sk_per_regime(DP,
// DYP) for the model, TP lanes at DP = 8, M lanes for the scores.  The cap counts TWO arrays and 256 lanes:
//   aesmc_switching_lookahead_conditional_max_particles(M, D, Dy) =
//       min( aesmc_switching_conditional_max_particles(D),
//            (160 KB / 8 - [TP + DP + 30 + M M + M per_regime + (DP == 8 ? 256 TP : 0) + 256 M]) / 2 )
// — K37's own cap for the models particle Gibbs is run on (8192 at M = 4, D = Dy = 4; 4096 at M = 4, D = Dy = 8), below it
// where the scores and the model take the room: 7918 at M = 16, D = Dy = 2, 3899 at M = 8 and 2139 at M = 16 with D = Dy = 8.
// 0 outside the family's limits.  Past the cap the provider composes the step from K32 and K37.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950), at 64 | 256 lanes per workgroup:
//   <DP,DYP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD  |  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2,2>       116      0        0             4       |    116      0        0             4
//   <2,4>       130      0        0             3       |    130      0        0             3
//   <2,8>       222      0        0             2       |    222      0        0             2
//   <4,2>       184      0        0             2       |    184      0        0             2
//   <4,4>       188      0        0             2       |    188      0        0             2
//   <4,8>       256      0        0             2       |    256      0        0             2
//   <8,2>       256     63        0             1       |    256     68        0             1       P in LDS
//   <8,4>       256     67        0             1       |    256     72        0             1       P in LDS
//   <8,8>       256     68        0             1       |    256     71        0             1       P in LDS
// and of the masked instantiations:
//   <2,2>       115      0        0             4       |    115      0        0             4
//   <2,4>       130      0        0             3       |    130      0        0             3
//   <2,8>       209      0        0             2       |    209      0        0             2
//   <4,2>       184      0        0             2       |    184      0        0             2
//   <4,4>       188      0        0             2       |    188      0        0             2
//   <4,8>       253      0        0             2       |    253      0        0             2
//   <8,2>       256     63        0             1       |    256     68        0             1       P in LDS
//   <8,4>       256     67        0             1       |    256     72        0             1       P in LDS
//   <8,8>       256     88        0             1       |    256     98        0             1       P in LDS
// No instantiation uses scratch, so none is excluded from the cap.  The registers are the larger of K32's loop and K37's pair
// score (which follow one another) plus what the row carries across both: the observation and the pointers.
//
// Measured (profiles/switching_lookahead_gibbs.txt; one MI355X, B = 1024, M = 4, us per call through the provider, medians)
// beside the composition K32 + K37 + K37 on zeros + torch.where; the same indices and K32's bits of log_weight and cdf:
//   D = Dy   K      K48      composition   |  without ancestor sampling: K48   K32 + K37
//   4        8        33.8       90.4       |                              28.7      46.0
//   4        64       26.9       92.5       |                              25.6      45.7
//   4        1024    206.1      253.8       |                             165.9     162.0
//   8        8       125.7      101.3       |                             105.3      68.8
//   8        64       97.8      119.5       |                              79.3      72.6
//   8        1024   1282.5     1486.6       |                            1046.1    1113.9
// Four shapes go the other way: D = 8, K = 8 (24 % slower, 53 % without ancestor sampling), D = 8, K = 64 and D = 4,
// K = 1024 without ancestor sampling (9 % and 2 %).  A workgroup per batch row leaves 8 of 64 lanes working at K = 8 and
// stages the model once per row, where K32 packs the particles into full workgroups (supposed from the geometry, not
// profiled).  DESIGN.md section 29 has the sweeps and what the look-ahead buys.
//
// K32's per-regime body is RESTATED below (switching_lookahead.hip is left as it was): a change to either copy belongs in
// both; tests/test_gpu_switching_lookahead_gibbs.py compares the two launches' outputs.
#include "ancestor_index.hpp"
#include "conditional_cdf.hpp"
#include "switching_host.hpp"
#include "switching_score.hpp"

namespace aesmc {

constexpr int kLcMaxWaves = 4;      // 256 lanes

struct LookaheadConditionalArgs {
  const double *log_Pi;             // [M,M]: the look-ahead's log-prior and the pinned score's transition term
  const double *A, *b, *q, *C, *d, *r;
  const int32_t *regime;            // [B,K] the stored system
  const double *mean, *cov;         // [B,K,D], [B,K,D(D+1)/2]
  const void *y;
  const uint8_t *observed;          // [B,Dy], nonzero = observed; NULL in the unmasked instantiations
  const double *u;                  // [B,K]
  const int32_t *regime_next;       // [B]
  const double *factor, *lambda;    // [B,D(D+1)/2], [B,D]; both NULL: no ancestor sampling
  int64_t *idx;                     // [B,K]
  double *log_weight, *cdf;         // [B,K], [B,K,M]
  int32_t *flags;
  int K, M, D, Dy, y_is_float, top;
};

// float64 words of a launch's LDS behind the two arrays: K37's (F, lam, the column of log Pi, the wavefronts' maxima, the
// totals, the wavefronts' ints), then log Pi, the model, for DP == 8 the [TP][lanes] covariances, the [M][lanes] scores
__host__ __device__ constexpr int lc_conditional_doubles(int dp) {
  return dp * (dp + 1) / 2 + dp + kSkMaxRegimes + 2 * kLcMaxWaves + 2 + kLcMaxWaves;
}
static inline size_t lc_fixed_doubles(int64_t M, int dp, int dyp, int lanes) {
  return (size_t)lc_conditional_doubles(dp) + (size_t)M * M + (size_t)M * sk_per_regime(dp, dyp) +
         (sk_cov_in_lds(dp) ? (size_t)dp * (dp + 1) / 2 * lanes : 0) + (size_t)M * lanes;
}
static inline int64_t lc_max_particles(int64_t M, int64_t D, int64_t Dy) {
  const int64_t words = 160 * 1024 / (int64_t)sizeof(double) - (int64_t)lc_fixed_doubles(M, sk_pad(D), sk_pad(Dy), kSkBlock);
  const int64_t fits = words > 0 ? words / 2 : 0, resampling = aesmc_switching_conditional_max_particles(D);
  return fits < resampling ? fits : resampling;
}

template <int DP, int DYP, int NT, bool Masked>
__global__ __launch_bounds__(NT) void switching_lookahead_conditional_kernel(const LookaheadConditionalArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lc_smem[];
  constexpr int kPer = sk_per_regime(DP, DYP);
  constexpr int TP = DP * (DP + 1) / 2, TY = DYP * (DYP + 1) / 2;
  constexpr int nwaves = NT / kWave;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int K = a.K, M = a.M, D = a.D, Dy = a.Dy;
  const int TD = D * (D + 1) / 2;
  const int64_t b = blockIdx.x;
  const bool pinned = a.factor != nullptr;
  double *free_c = lc_smem, *pin_c = lc_smem + K;
  double *Ft = lc_smem + (pinned ? 2 : 1) * (size_t)K;      // [TP]
  double *lt = Ft + TP;                                     // [DP]
  double *pt = lt + DP;                                     // [kSkMaxRegimes]: log Pi[s, s'] by s
  double(*wave_max)[kLcMaxWaves] = reinterpret_cast<double(*)[kLcMaxWaves]>(pt + kSkMaxRegimes);      // [2][waves]
  double *totals = pt + kSkMaxRegimes + 2 * kLcMaxWaves;    // [2]
  int(*wave_int)[kLcMaxWaves] = reinterpret_cast<int(*)[kLcMaxWaves]>(totals + 2);                    // [2][waves]
  double *lp = reinterpret_cast<double *>(wave_int + 2);    // [M * M]
  double *mdl = lp + M * M;                                 // [M * kPer]
  double *cov_lds = mdl + M * kPer + tid;                   // DP == 8: [TP][NT], the lane's column
  double *scores = mdl + M * kPer + (sk_cov_in_lds(DP) ? TP * NT : 0) + tid;      // [M][NT], the lane's column
  const double nan = Num<double>::nan(), inf = Num<double>::pos_inf();

  for (int e = tid; e < M * M; e += NT) lp[e] = a.log_Pi[e];
  sk_stage_model<DP, DYP, NT>(mdl, M, D, Dy, a.A, a.b, a.q, a.C, a.d, a.r);
  if (pinned) {      // the reference's (F, lam) and its column of log Pi (K37's)
    for (int e = tid; e < TP; e += NT) Ft[e] = e < TD ? a.factor[b * TD + e] : 0.0;
    for (int e = tid; e < DP; e += NT) lt[e] = e < D ? a.lambda[b * D + e] : 0.0;
    const int next = a.regime_next[b];
    const bool outside = next < 0 || next >= M;      // (a NaN column: every score of the row is NaN)
    if (outside && tid == 0) raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    for (int s = tid; s < M; s += NT) pt[s] = outside ? nan : a.log_Pi[s * M + next];
  }
  __syncthreads();

  // ---- the row's observation (K32's, K40's) -----------------------------------------------------------------------------------
  double yv[DYP];
  if (a.y_is_float) {
    const float *yrow = (const float *)a.y + b * Dy;
#pragma unroll
    for (int i = 0; i < DYP; ++i) yv[i] = i < Dy ? (double)yrow[i] : 0.0;
  } else {
    const double *yrow = (const double *)a.y + b * Dy;
#pragma unroll
    for (int i = 0; i < DYP; ++i) yv[i] = i < Dy ? yrow[i] : 0.0;
  }
  bool ob[DYP];
  int n_obs = Dy;
  if constexpr (Masked) {
    const uint8_t *orow = a.observed + b * Dy;
    n_obs = 0;
#pragma unroll
    for (int i = 0; i < DYP; ++i) {
      ob[i] = i < Dy ? orow[i] != 0 : false;
      n_obs += ob[i] ? 1 : 0;
      yv[i] = ob[i] ? yv[i] : 0.0;      // (may be NaN or Inf where not observed)
    }
  } else {
#pragma unroll
    for (int i = 0; i < DYP; ++i) ob[i] = true;
  }

  // ---- per particle: the look-ahead, then the pinned score; the maxima and NaN markers of both ------------------------------------
  double m_free = -__builtin_huge_val(), m_pin = -__builtin_huge_val();
  int nan_free = 0, nan_pin = 0;
#pragma clang loop unroll(disable)
  for (int k = tid; k < K; k += NT) {
    const int64_t n = b * K + k;
    double *crow = a.cdf + n * M;
    const double *mrow = a.mean + n * D, *prow = a.cov + n * TD;
    const int s_prev = a.regime[n];
    const bool known = s_prev >= 0 && s_prev < M;
    double x = nan;      // the first-stage log-weight
    if (!known) {
      raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    } else {
      const double *prior = lp + s_prev * M;
      double mp[DP];
      SkCov<TP, sk_cov_in_lds(DP), NT> Pm;
      Pm.lds = cov_lds;
#pragma clang loop unroll(disable)
      for (int j = 0; j < M; ++j) {
        const double *Am = mdl + j * kPer, *bv = Am + DP * DP, *q2 = bv + DP, *Cm = q2 + DP, *dv = Cm + DYP * DP, *r2 = dv + DYP;

        // ---- predict (K31's) ---------------------------------------------------------------------------------------------------
        {
          double mi[DP], Pi[TP];
#pragma unroll
          for (int i = 0; i < DP; ++i) mi[i] = i < D ? mrow[i] : 0.0;
#pragma unroll
          for (int e = 0; e < TP; ++e) Pi[e] = e < TD ? prow[e] : 0.0;
#pragma unroll
          for (int i = 0; i < DP; ++i) {
            double acc = bv[i];
#pragma unroll
            for (int l = 0; l < DP; ++l) acc = __builtin_fma(Am[i * DP + l], mi[l], acc);
            mp[i] = acc;
          }
          double W[DP][DP];      // A P: row i from row i of A alone
#pragma unroll
          for (int i = 0; i < DP; ++i) {
#pragma unroll
            for (int l = 0; l < DP; ++l) {
              double acc = 0.0;
#pragma unroll
              for (int c = 0; c < DP; ++c) acc = __builtin_fma(Am[i * DP + c], Pi[sk_tri(c, l)], acc);
              W[i][l] = acc;
            }
          }
          SK_REREAD_LDS();
#pragma unroll
          for (int i = 0; i < DP; ++i) {
#pragma unroll
            for (int c = 0; c <= i; ++c) {
              double acc = i == c ? q2[i] : 0.0;
#pragma unroll
              for (int l = 0; l < DP; ++l) acc = __builtin_fma(Am[i * DP + l], W[c][l], acc);
              Pm.set(sk_tri(i, c), acc);
            }
          }
        }

        // ---- innovation, U = C P-, S_ic = C_i . U_c + diag(r^2) (K31's) -------------------------------------------------------
        SK_REREAD_LDS();
        double e[DYP], U[DYP][DP], S[TY];
#pragma unroll
        for (int i = 0; i < DYP; ++i) {
          if (i) SK_REREAD_LDS();
          double acc = yv[i] - dv[i];
#pragma unroll
          for (int l = 0; l < DP; ++l) acc = __builtin_fma(-Cm[i * DP + l], mp[l], acc);
          e[i] = Masked && !ob[i] ? 0.0 : acc;
#pragma unroll
          for (int l = 0; l < DP; ++l) {
            double w = 0.0;
#pragma unroll
            for (int c = 0; c < DP; ++c) w = __builtin_fma(Cm[i * DP + c], Pm.get(sk_tri(c, l)), w);
            U[i][l] = Masked && !ob[i] ? 0.0 : w;
          }
#pragma unroll
          for (int c = 0; c <= i; ++c) {
            double w = i == c ? r2[i] : 0.0;
#pragma unroll
            for (int l = 0; l < DP; ++l) w = __builtin_fma(Cm[i * DP + l], U[c][l], w);
            S[sk_tri(i, c)] = Masked && !(ob[i] && ob[c]) ? (i == c ? 1.0 : 0.0) : w;
          }
        }

        // ---- Lam = chol(S) in place, column by column; inv[c] = 1 / Lam_cc (K31's) -----------------------------------------------
        double inv[DYP], log_det = 0.0;
        bool positive = true;
#pragma unroll
        for (int c = 0; c < DYP; ++c) {
          double pivot = S[sk_tri(c, c)];
#pragma unroll
          for (int h = 0; h < c; ++h) pivot = __builtin_fma(-S[sk_tri(c, h)], S[sk_tri(c, h)], pivot);
          positive = positive && pivot > 0.0;
          const double lcc = __builtin_sqrt(pivot);
          S[sk_tri(c, c)] = lcc;
          inv[c] = 1.0 / lcc;
          log_det += ::log(lcc);
#pragma unroll
          for (int i = c + 1; i < DYP; ++i) {
            double acc = S[sk_tri(i, c)];
#pragma unroll
            for (int h = 0; h < c; ++h) acc = __builtin_fma(-S[sk_tri(i, h)], S[sk_tri(c, h)], acc);
            S[sk_tri(i, c)] = acc * inv[c];
          }
        }

        // ---- v = Lam^-1 e and the score (K32's) ------------------------------------------------------------------------------------
        double quad = 0.0;
#pragma unroll
        for (int i = 0; i < DYP; ++i) {
          double acc = e[i];
#pragma unroll
          for (int c = 0; c < i; ++c) acc = __builtin_fma(-S[sk_tri(i, c)], e[c], acc);
          e[i] = acc * inv[i];
          quad = __builtin_fma(e[i], e[i], quad);
        }
        const double ell = (-0.5 * quad - log_det) - (double)n_obs * kHalfLog2Pi;
        const double lpj = prior[j];
        // a regime of prior probability 0 has the score -inf whatever its pivots are; elsewhere a pivot that is not positive is NaN
        scores[j * NT] = lpj == -inf ? -inf : positive ? lpj + ell : nan;
      }

      // ---- log_w = logsumexp_j g_j; cdf_j = sum_{i <= j} exp(g_i - log_w), exactly 1 from the last positive term onwards (K32's) ----
      double top = -inf;
      bool invalid = false;
      for (int j = 0; j < M; ++j) {
        const double g = scores[j * NT];
        invalid = invalid || g != g;
        top = g > top ? g : top;
      }
      if (!(invalid || !(top > -inf))) {
        double sum = 0.0;
        for (int j = 0; j < M; ++j) sum += ::exp(scores[j * NT] - top);
        x = top + ::log(sum);
        int last = 0;
        for (int j = 0; j < M; ++j) {
          const double p = ::exp(scores[j * NT] - x);
          scores[j * NT] = p;
          last = p > 0.0 ? j : last;
        }
        double running = 0.0;
        for (int j = 0; j < M; ++j) {
          running += scores[j * NT];
          crow[j] = j >= last ? 1.0 : running;
        }
      }
    }
    a.log_weight[n] = x;
    if (x != x)
      for (int j = 0; j < M; ++j) crow[j] = nan;
    nan_free |= (x != x);
    m_free = fmax(m_free, x);      // (fmax drops a NaN operand: the marker keeps it)
    free_c[k] = x;

    if (pinned) {      // K37's pinned score of the EQUALLY weighted system: the log-weight is 0.0
      double score = nan;
      if (known) {
        double m[DP];
        SkCov<TP, sk_cov_in_lds(DP), NT> P;
        P.lds = cov_lds;
#pragma unroll
        for (int i = 0; i < DP; ++i) m[i] = i < D ? mrow[i] : 0.0;
#pragma unroll
        for (int e = 0; e < TP; ++e) P.set(e, e < TD ? prow[e] : 0.0);
        score = switching_pair_score<DP>(Ft, lt, m, P, pt + s_prev, 0.0, true);
      }
      nan_pin |= (score != score);
      m_pin = fmax(m_pin, score);
      pin_c[k] = score;
    }
  }

  // ---- K37's tail from here on ---------------------------------------------------------------------------------------------------
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

  // ---- weights in place, and the last particle of positive weight ------------------------------------------------------------------
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

  // ---- the CDFs: front to back, one lane each — in two wavefronts, side by side, when the workgroup has two ----------------------
  const int pin_lane = NT > kWave ? kWave : 0;
  if (tid == 0) totals[0] = running_sum_in_place(free_c, K);
  if (scan_pin && tid == pin_lane) totals[1] = running_sum_in_place(pin_c, K);
  __syncthreads();
  for (int w = 0; w < nwaves; ++w) {
    last_free = max(last_free, wave_int[0][w]);
    last_pin = max(last_pin, wave_int[1][w]);
  }

  // ---- one bisection per slot ------------------------------------------------------------------------------------------------------
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

// K48, and its masked entry (`masked`: observed [B,Dy] given): one set of checks, one launch
static int lc_step(bool masked, const uint8_t *observed, int y_dtype, const aesmc_switching_model *model, const double *log_Pi,
                   const int32_t *regime, const double *mean, const double *cov, const void *y, const double *u,
                   const int32_t *regime_next, const double *factor, const double *lambda, int64_t *out_idx,
                   double *log_weight, double *cdf, int32_t *flags, int64_t B, int64_t K, void *stream) {
  if (masked && observed == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  if (model == nullptr || log_Pi == nullptr || regime == nullptr || mean == nullptr || cov == nullptr || u == nullptr ||
      out_idx == nullptr || log_weight == nullptr || cdf == nullptr || B < 0 || K < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool pinned = factor != nullptr;
  if (pinned != (lambda != nullptr) || (pinned && regime_next == nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_observation(y, y_dtype) || !sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, false))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(log_Pi, 8) || !sk_aligned(regime, 4) || !sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(u, 8) ||
      !sk_aligned(regime_next, 4) || !sk_aligned(factor, 8) || !sk_aligned(lambda, 8) || !sk_aligned(out_idx, 8) ||
      !sk_aligned(log_weight, 8) || !sk_aligned(cdf, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({out_idx, log_weight, cdf},
                           {log_Pi, regime, mean, cov, y, u, regime_next, factor, lambda, masked ? observed : nullptr}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (!sk_extents_supported(model->M, model->D, model->Dy) || K > lc_max_particles(model->M, model->D, model->Dy) ||
      !sk_fits_32bit(B, K, kSkTriMax))
    return AESMC_ERR_UNSUPPORTED;
  LookaheadConditionalArgs a;
  sk_fill_model(a, model);
  a.log_Pi = log_Pi, a.regime = regime, a.mean = mean, a.cov = cov, a.y = y;
  a.observed = masked ? observed : nullptr;
  a.u = u, a.regime_next = regime_next, a.factor = factor, a.lambda = lambda;
  a.idx = out_idx, a.log_weight = log_weight, a.cdf = cdf, a.flags = flags;
  a.K = (int)K;
  a.y_is_float = y_dtype == AESMC_F32;
  a.top = bisection_top(K);
  const int dp = sk_pad(model->D), dyp = sk_pad(model->Dy);
  const int lanes = K <= kWave ? kWave : kSkBlock;
  const size_t lds = ((size_t)K * (pinned ? 2 : 1) + lc_fixed_doubles(a.M, dp, dyp, lanes)) * sizeof(double);
  return sk_for_extents(dp, dyp, [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      constexpr int DP = decltype(d)::value, DYP = decltype(dy)::value;
      constexpr bool kMasked = decltype(m)::value;
      return lanes == kWave ? sk_launch(&switching_lookahead_conditional_kernel<DP, DYP, kWave, kMasked>, dim3((unsigned)B),
                                        dim3(kWave), lds, (hipStream_t)stream, a)
                            : sk_launch(&switching_lookahead_conditional_kernel<DP, DYP, kSkBlock, kMasked>, dim3((unsigned)B),
                                        dim3(kSkBlock), lds, (hipStream_t)stream, a);
    });
  });
}

}  // namespace aesmc

extern "C" int64_t aesmc_switching_lookahead_conditional_max_particles(int64_t M, int64_t D, int64_t Dy) {
  using namespace aesmc;
  return !sk_extents_positive(M, D, Dy) || !sk_extents_supported(M, D, Dy) ? 0 : lc_max_particles(M, D, Dy);
}

extern "C" int aesmc_switching_lookahead_conditional_ancestor_index(
    int y_dtype, const aesmc_switching_model *model, const double *log_Pi, const int32_t *regime, const double *mean,
    const double *cov, const void *y, const double *u, const int32_t *regime_next, const double *factor, const double *lambda,
    int64_t *out_idx, double *log_weight, double *cdf, int32_t *flags, int64_t B, int64_t K, void *stream) {
  return aesmc::lc_step(false, nullptr, y_dtype, model, log_Pi, regime, mean, cov, y, u, regime_next, factor, lambda, out_idx,
                        log_weight, cdf, flags, B, K, stream);
}

extern "C" int aesmc_switching_masked_lookahead_conditional_ancestor_index(
    int y_dtype, const aesmc_switching_model *model, const double *log_Pi, const int32_t *regime, const double *mean,
    const double *cov, const void *y, const uint8_t *observed, const double *u, const int32_t *regime_next,
    const double *factor, const double *lambda, int64_t *out_idx, double *log_weight, double *cdf, int32_t *flags, int64_t B,
    int64_t K, void *stream) {
  return aesmc::lc_step(true, observed, y_dtype, model, log_Pi, regime, mean, cov, y, u, regime_next, factor, lambda, out_idx,
                        log_weight, cdf, flags, B, K, stream);
}
