// The look-ahead of the fully adapted Rao-Blackwellised filter (mixture Kalman filter with the regimes drawn from their exact
// posterior; Chen & Liu 2000; Doucet, Gordon & Krishnamurthy 2001; the auxiliary particle filter of Pitt & Shephard 1999)
// for a switching linear-Gaussian state-space model — aesmc_switching_lookahead (K32) of include/aesmc_hip.h.
//
// Particle k of batch row b carries (s, m, P).  One launch gives it, from ONE Kalman prediction per regime j, the scores
// g_j = log Pi[s, j] + log p(y | s_t = j, history), their log-sum-exp — the exact first-stage weight log p(y | history) —
// and the cumulative row of the exact regime posterior, which K33 (switching_kalman.hip) draws the regime from.
//
//   workgroup = 256 consecutive particles of the flattened [B K] range, one lane per particle;
//   model     staged as K31 stages it (switching_kalman.hpp), the rows of log Pi (step 0: log pi0) in front of it;
//   regimes   a RUN-TIME loop over j: every lane of a wavefront reads regime j's block together, so every LDS read of the
//             model is a broadcast (K31 pays a bank conflict per distinct regime among its lanes);
//   per j     K31's predict, U = C P-, S, the Cholesky factor and the ONE solve for the innovation, in K31's order and as
//             the same float64 fma chains; neither Lam^-1 U nor the downdate.  The lane's state is read inside the loop (the
//             compiler hoists what it has registers for); the 8-wide instantiations keep P- in LDS as K31 does;
//   scores    g_j goes to LDS [M][256] (a register array indexed by j would go to scratch); three short passes over j read
//             them back: the maximum, the sum of exponentials, and the running sum of exp(g_j - log_w);
//   LDS       at M = 16, D = Dy = 8: 2 KB (log Pi) + 20 KB (model) + 72 KB (P-) + 32 KB (scores) = 126 KB of the 160 KB.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP,DYP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2,2>        68      0        0             7
//   <2,4>        94      0        0             5
//   <2,8>       166      0        0             3
//   <4,2>       100      0        0             4
//   <4,4>       124      0        0             4
//   <4,8>       206      0        0             2
//   <8,2>       256     22        0             1       P- in LDS
//   <8,4>       256     26        0             1       P- in LDS
//   <8,8>       256     34        0             1       P- in LDS
// and of the masked instantiations (K40, aesmc_switching_masked_lookahead: K39's selections per regime):
//   <2,2>        69      0        0             7
//   <2,4>        91      0        0             5
//   <2,8>       163      0        0             3
//   <4,2>       103      0        0             4
//   <4,4>       124      0        0             4
//   <4,8>       217      0        0             2
//   <8,2>       256     22        0             1       P- in LDS
//   <8,4>       256     26        0             1       P- in LDS
//   <8,8>       256     82        0             1       P- in LDS
// and of the scores instantiations (K43, aesmc_switching_lookahead_scores: g_j itself in place of the cumulative row — the body
// up to log_w, then nothing), unmasked | masked:
//   <2,2>        66      0        0             7       |     66      0        0             7
//   <2,4>        88      0        0             5       |     89      0        0             5
//   <2,8>       164      0        0             3       |    161      0        0             3
//   <4,2>       102      0        0             4       |    101      0        0             4
//   <4,4>       116      0        0             4       |    122      0        0             4
//   <4,8>       204      0        0             2       |    215      0        0             2
//   <8,2>       256     20        0             1       |    256     20        0             1       P- in LDS
//   <8,4>       256     24        0             1       |    256     24        0             1       P- in LDS
//   <8,8>       256     32        0             1       |    256     80        0             1       P- in LDS
// (the K32 and K40 lines above are unchanged by the further template parameter).
// No instantiation spills: without V = Lam^-1 U and the downdate the live set of <8,8> (U 128, S 72 registers and the
// vectors) fits, and the input covariance is read again per regime instead of being held across the loop.
//
// Traffic per particle at D = Dy = 4, M = 4: 4 + 32 + 80 (state) + 8 (log-weight) + 32 (CDF row) = 156 bytes; at D = 8:
// 4 + 64 + 288 + 8 + 32 = 396 bytes (the state's re-reads per regime are served by the caches).
#include "switching_host.hpp"

namespace aesmc {

struct LookaheadArgs {
  const double *log_prior;          // [M,M] (later steps) or [M] (step 0)
  const double *m0, *s0;            // [D]
  const double *A, *b, *q, *C, *d, *r;
  const int32_t *regime_in;         // NULL: step 0
  const double *mean_in, *cov_in;
  const void *y;
  const uint8_t *observed;          // K40: [B,Dy], nonzero = observed; NULL in the unmasked instantiations
  double *log_weight, *cdf;
  int32_t *flags;
  int64_t N;
  uint32_t K;
  int M, D, Dy, y_is_float;
};

// LDS: [M * M] (or [M]) log-priors, the model (M blocks of sk_per_regime values), for DP == 8 [TP][256] predicted
// covariances, then [M][256] scores
// Masked (K40): K39's three selections (switching_kalman.hip) for every regime; the constant counts the observed components
// Scores (K43): the row that a.cdf points at receives g_j itself, as computed, and no cumulative row
template <int DP, int DYP, bool Masked, bool Scores>
__global__ __launch_bounds__(kSkBlock) void switching_lookahead_kernel(const LookaheadArgs a) {
  extern __shared__ __attribute__((aligned(16))) double la_smem[];
  constexpr int kPer = sk_per_regime(DP, DYP);
  constexpr int TP = DP * (DP + 1) / 2, TY = DYP * (DYP + 1) / 2;
  const int M = a.M, D = a.D, Dy = a.Dy;
  const bool later = a.regime_in != nullptr;
  const int nlp = later ? M * M : M;
  double *lp = la_smem;
  double *mdl = la_smem + nlp;
  double *scores = mdl + M * kPer + (sk_cov_in_lds(DP) ? TP * kSkBlock : 0) + threadIdx.x;      // the lane's column
  for (int e = threadIdx.x; e < nlp; e += kSkBlock) lp[e] = a.log_prior[e];
  sk_stage_model<DP, DYP>(mdl, M, D, Dy, a.A, a.b, a.q, a.C, a.d, a.r);
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (n >= a.N) return;
  const int64_t b = n / a.K;
  const int TD = D * (D + 1) / 2;
  const double nan = Num<double>::nan(), inf = Num<double>::pos_inf();
  double *crow = a.cdf + n * M;

  int s_prev = 0;
  if (later) {
    s_prev = a.regime_in[n];
    if (s_prev < 0 || s_prev >= M) {
      raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
      a.log_weight[n] = nan;
      for (int j = 0; j < M; ++j) crow[j] = nan;
      return;
    }
  }
  const double *prior = lp + (later ? s_prev * M : 0);

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

  double mp[DP];
  SkCov<TP, sk_cov_in_lds(DP)> Pm;
  Pm.lds = mdl + M * kPer + threadIdx.x;
  if (!later) {      // the prior is every regime's prediction
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      mp[i] = i < D ? a.m0[i] : 0.0;
      const double s0 = i < D ? a.s0[i] : 0.0;
#pragma unroll
      for (int j = 0; j <= i; ++j) Pm.set(sk_tri(i, j), i == j ? s0 * s0 : 0.0);
    }
  }

#pragma clang loop unroll(disable)
  for (int j = 0; j < M; ++j) {
    const double *Am = mdl + j * kPer, *bv = Am + DP * DP, *q2 = bv + DP, *Cm = q2 + DP, *dv = Cm + DYP * DP, *r2 = dv + DYP;

    // ---- predict (K31's) -------------------------------------------------------------------------------------------------
    if (later) {
      double mi[DP], Pi[TP];
      const double *mrow = a.mean_in + n * D, *prow = a.cov_in + n * TD;
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

    // ---- innovation, U = C P-, S_ic = C_i . U_c + diag(r^2) (K31's) -----------------------------------------------------
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

    // ---- Lam = chol(S) in place, column by column; inv[c] = 1 / Lam_cc (K31's) ---------------------------------------------
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

    // ---- v = Lam^-1 e and the score -------------------------------------------------------------------------------------------
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
    const double g = lpj == -inf ? -inf : positive ? lpj + ell : nan;
    scores[j * kSkBlock] = g;
    if constexpr (Scores) crow[j] = g;
  }

  // ---- log_w = logsumexp_j g_j; cdf_j = sum_{i <= j} exp(g_i - log_w), exactly 1 from the last positive term onwards -------------
  double top = -inf;
  bool invalid = false;
  for (int j = 0; j < M; ++j) {
    const double g = scores[j * kSkBlock];
    invalid = invalid || g != g;
    top = g > top ? g : top;
  }
  if (invalid || !(top > -inf)) {      // (no regime of positive prior: the host's validation excludes it)
    a.log_weight[n] = nan;
    if constexpr (!Scores)
      for (int j = 0; j < M; ++j) crow[j] = nan;
    return;
  }
  double sum = 0.0;
  for (int j = 0; j < M; ++j) sum += ::exp(scores[j * kSkBlock] - top);
  const double log_w = top + ::log(sum);
  a.log_weight[n] = log_w;
  if constexpr (Scores) return;
  int last = 0;
  for (int j = 0; j < M; ++j) {
    const double p = ::exp(scores[j * kSkBlock] - log_w);
    scores[j * kSkBlock] = p;
    last = p > 0.0 ? j : last;
  }
  double running = 0.0;
  for (int j = 0; j < M; ++j) {
    running += scores[j * kSkBlock];
    crow[j] = j >= last ? 1.0 : running;
  }
}

// K32, and K40 (`masked`: observed [B,Dy] given), and K43 (`scores`: `cdf` receives the scores): one set of checks, one launch
static int la_step(bool scores, bool masked, const uint8_t *observed, int y_dtype, const aesmc_switching_model *model,
                   const double *log_prior, const int32_t *regime_in, const double *mean_in, const double *cov_in,
                   const void *y, double *log_weight, double *cdf, int32_t *flags, int64_t B, int64_t K, void *stream) {
  if (masked && observed == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  if (model == nullptr || log_prior == nullptr || log_weight == nullptr || cdf == nullptr || B < 0 || K < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool later = regime_in != nullptr;
  if (later != (mean_in != nullptr) || later != (cov_in != nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_observation(y, y_dtype) || !sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, true))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(log_prior, 8) || !sk_aligned(regime_in, 4) || !sk_aligned(mean_in, 8) || !sk_aligned(cov_in, 8) ||
      !sk_aligned(log_weight, 8) || !sk_aligned(cdf, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({log_weight, cdf}, {mean_in, cov_in, observed})) return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (!sk_extents_supported(model->M, model->D, model->Dy) || !sk_fits_32bit(B, K, kSkTriMax)) return AESMC_ERR_UNSUPPORTED;
  LookaheadArgs a;
  sk_fill_model(a, model);
  a.log_prior = log_prior;
  a.m0 = model->m0, a.s0 = model->s0;
  a.regime_in = regime_in, a.mean_in = mean_in, a.cov_in = cov_in, a.y = y;
  a.observed = masked ? observed : nullptr;
  a.log_weight = log_weight, a.cdf = cdf, a.flags = flags;
  a.N = B * K, a.K = (uint32_t)K;
  a.y_is_float = y_dtype == AESMC_F32;
  const int dp = sk_pad(model->D), dyp = sk_pad(model->Dy);
  const size_t lds = ((later ? (size_t)a.M * a.M : (size_t)a.M) + (size_t)a.M * sk_per_regime(dp, dyp) +
                      (sk_cov_in_lds(dp) ? dp * (dp + 1) / 2 * kSkBlock : 0) + (size_t)a.M * kSkBlock) * sizeof(double);
  return sk_for_extents(dp, dyp, [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      return sk_for_flag(scores, [&](auto sc) {
        return sk_launch(&switching_lookahead_kernel<decltype(d)::value, decltype(dy)::value, decltype(m)::value, decltype(sc)::value>,
                         sk_grid(a.N), dim3(kSkBlock), lds, (hipStream_t)stream, a);
      });
    });
  });
}

}  // namespace aesmc

extern "C" int aesmc_switching_lookahead(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                                         const int32_t *regime_in, const double *mean_in, const double *cov_in, const void *y,
                                         double *log_weight, double *cdf, int32_t *flags, int64_t B, int64_t K, void *stream) {
  return aesmc::la_step(false, false, nullptr, y_dtype, model, log_prior, regime_in, mean_in, cov_in, y, log_weight, cdf, flags, B, K,
                        stream);
}

extern "C" int aesmc_switching_masked_lookahead(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                                                const int32_t *regime_in, const double *mean_in, const double *cov_in,
                                                const void *y, const uint8_t *observed, double *log_weight, double *cdf,
                                                int32_t *flags, int64_t B, int64_t K, void *stream) {
  return aesmc::la_step(false, true, observed, y_dtype, model, log_prior, regime_in, mean_in, cov_in, y, log_weight, cdf, flags, B, K,
                        stream);
}

extern "C" int aesmc_switching_lookahead_scores(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                                                const int32_t *regime_in, const double *mean_in, const double *cov_in,
                                                const void *y, double *scores, double *log_weight, int32_t *flags, int64_t B,
                                                int64_t K, void *stream) {
  return aesmc::la_step(true, false, nullptr, y_dtype, model, log_prior, regime_in, mean_in, cov_in, y, log_weight, scores, flags,
                        B, K, stream);
}

extern "C" int aesmc_switching_masked_lookahead_scores(int y_dtype, const aesmc_switching_model *model,
                                                       const double *log_prior, const int32_t *regime_in,
                                                       const double *mean_in, const double *cov_in, const void *y,
                                                       const uint8_t *observed, double *scores, double *log_weight,
                                                       int32_t *flags, int64_t B, int64_t K, void *stream) {
  return aesmc::la_step(true, true, observed, y_dtype, model, log_prior, regime_in, mean_in, cov_in, y, log_weight, scores, flags,
                        B, K, stream);
}
