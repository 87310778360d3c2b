// One step of the Rao-Blackwellised particle filter (mixture Kalman filter; Doucet, de Freitas, Murphy & Russell 2000; Chen &
// Liu 2000) for a switching linear-Gaussian state-space model — aesmc_switching_kalman_step (K31) of include/aesmc_hip.h.
//
// The same kernel is aesmc_switching_kalman_draw (K33): one more pointer, `particle_cdf`, from whose row at the ancestor's
// position the regime is drawn instead of from the chain's rows (the fully adapted filter: switching_lookahead.hip writes
// those rows).  NULL for K31, whose arithmetic and order it does not touch.
//
// And aesmc_switching_kalman_conditional_step (K38), the step of a conditional sweep (particle Gibbs on the regimes): one more
// pointer, `pinned_regime` [B], whose entry slot K-1 of the row takes as its regime in place of the draw — the reference
// path's.  NULL for K31 and K33; everything after the regime is chosen is the same code for every slot.
//
// And aesmc_switching_kalman_conditional_draw (K49), the step of a LOOK-AHEAD conditional sweep: both pointers at once — the
// free slots draw from their ancestors' rows as K33's, slot K-1 takes the pinned regime as K38's.  The kernel always took
// the two together (the masked entry passes both); K49 is the unmasked entry that does.
//
// And aesmc_switching_kalman_masked_step (K39), any of the three under a mask of the observation's components: the kernel's
// second instantiation per extent (`Masked`), in which a component that batch row b did not observe is deleted from the step
// by three selections placed after the chains of the unmasked text — see the kernel's comment.  The unmasked instantiations
// are compiled from the text they had before K39.
//
// Only the regimes are sampled.  Particle k of batch row b carries (s, m, P): its regime and the exact Kalman mean and
// covariance of the continuous state given its regime history.  One launch, per particle: the gather through the ancestors,
// the inverse-CDF regime draw, the Kalman predict, the Dy x Dy Cholesky factor of the innovation covariance, two triangular
// solves, the rank-Dy downdate and the predictive log-likelihood, which is the particle's weight.
//
//   workgroup = 256 consecutive particles of the flattened [B K] range, one lane per particle;
//   model     every regime's A, b, q^2, C, d, r^2 and the cumulative rows of the chain staged once per workgroup into LDS
//             as float64, zero-padded to the instantiation's extents (r^2 padded with ONE: the padded pivots are 1, their
//             logarithms 0) — 20 KB + 2 KB at M = 16, D = Dy = 8; a lane reads the block of ITS regime (a broadcast where
//             the lanes of a wavefront agree, a bank conflict per distinct regime where they do not);
//   state     the lane's m, P (packed lower triangle), the innovation covariance S and V = Lam^-1 C P- live in registers;
//             the kernel is templated on the padded extents DP of D and DYP of Dy (2, 4, 8 each), all loops fully unrolled;
//             the predict forms W = A P and then P-_ij = A_i . W_j, the innovation U = C P- and S_ij = C_i . U_j: each row
//             of A and C serves one block of the code and is read from LDS again in the next (SK_REREAD_LDS);
//   chains    every value is ONE chain of float64 __builtin_fma in the header's order.  A padded term multiplies a zero by a
//             zero: the chain's bits do not change.  One reciprocal per pivot; no atomics but the flag's.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP,DYP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2,2>        64      0        0             7
//   <2,4>        95      0        0             5
//   <2,8>       208      0        0             2
//   <4,2>        89      0        0             5
//   <4,4>       147      0        0             3
//   <4,8>       256     92        0             1
//   <8,2>       256      0        0             2       P- in LDS
//   <8,4>       256      0        0             2       P- in LDS
//   <8,8>       256    256      132             1       P- in LDS
// and of the masked instantiations (K39, aesmc_switching_kalman_masked_step: `Masked` below):
//   <2,2>        65      0        0             7
//   <2,4>        95      0        0             5
//   <2,8>       208      0        0             2
//   <4,2>        90      0        0             5
//   <4,4>       148      0        0             3
//   <4,8>       256     54        0             1
//   <8,2>       256      0        0             2       P- in LDS
//   <8,4>       256      0        0             2       P- in LDS
//   <8,8>       256    242        0             1       P- in LDS
// (the masked <8,8> uses no scratch where the unmasked one takes 132 bytes: the register allocator's outcome on the text
// with the selections in it, not something the kernel was shaped for; profiles/switching_missing.txt has both forms' times.)
// With P- in registers <8,8> took 328 bytes of scratch per lane (its live set — V 128, S 72, P- 72 registers and the vectors —
// exceeds the 256 architectural VGPRs; the accumulation registers are a spill space with a move per use), so the 8-wide
// instantiations keep the packed P- in LDS in an [element][lane] layout (72 KB per workgroup).  <8,8> still spills 33
// dwords per lane and moves through the accumulation registers (about 880 moves beside 755 multiply-adds): slower than
// it could be, correct, and measured as it is (profiles/switching_kalman.txt).
//
// Traffic per particle at D = Dy = 4: 8 (ancestor) + 8 (uniform) + 2 (4 + 32 + 80) (state in and out) + 8 (log-weight) =
// 256 bytes; at D = 8: 736 bytes.
#include "switching_host.hpp"

namespace aesmc {

struct SwitchingArgs {
  const double *cdf;                // [M,M] (later steps) or [M] (step 0); not read when particle_cdf is given
  const double *particle_cdf;       // K33: [B,K,M], the row of the ancestor's position; NULL: K31
  const int32_t *pinned_regime;     // K38: [B], the regime of slot K-1; NULL: K31, K33
  const double *m0, *s0;            // [D]
  const double *A, *b, *q, *C, *d, *r;
  const int32_t *regime_in;         // NULL: step 0
  const double *mean_in, *cov_in;
  const int64_t *idx;
  const double *uniforms;
  const void *y;
  const uint8_t *observed;          // K39: [B,Dy], nonzero = observed; NULL in the unmasked instantiations
  int32_t *regime_out;
  double *mean_out, *cov_out, *log_weight;
  int32_t *flags;
  int64_t N;
  uint32_t K;
  int M, D, Dy, y_is_float;
};

// LDS: [M * M] (or [M]) cumulative rows, then per regime kPer values: A [DP,DP], b [DP], q^2 [DP], C [DYP,DP], d [DYP],
// r^2 [DYP]; then, for DP == 8, [TP][256] predicted covariances
// Masked (K39): a component whose byte of `observed` is zero is deleted from the step — its e, its row of U and its row and
// column of S are SELECTED to 0, 0 and the identity's after their chains (its y is never read into one), so that its pivot is
// 1 as a padded component's is; the constant counts the observed components
template <int DP, int DYP, bool Masked>
__global__ __launch_bounds__(kSkBlock) void switching_kalman_kernel(const SwitchingArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sk_smem[];
  constexpr int kPer = DP * DP + 2 * DP + DYP * DP + 2 * DYP;
  constexpr int TP = DP * (DP + 1) / 2, TY = DYP * (DYP + 1) / 2;
  const int M = a.M, D = a.D, Dy = a.Dy;
  const bool later = a.regime_in != nullptr;
  const int ncdf = a.particle_cdf != nullptr ? 0 : later ? M * M : M;
  double *cdf = sk_smem;
  double *mdl = sk_smem + ncdf;
  for (int e = threadIdx.x; e < ncdf; e += kSkBlock) cdf[e] = a.cdf[e];
  sk_stage_model<DP, DYP>(mdl, M, D, Dy, a.A, a.b, a.q, a.C, a.d, a.r);
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (n >= a.N) return;
  const int64_t b = n / a.K;
  const int64_t k = n - b * a.K;
  const int TD = D * (D + 1) / 2;

  // ---- the ancestor and the regime ------------------------------------------------------------------------------------
  const int64_t anc = (later && a.idx != nullptr) ? a.idx[n] : k;
  bool good = anc >= 0 && anc < (int64_t)a.K;
  const int64_t src = b * a.K + (good ? anc : 0);
  int s_prev = 0;
  if (later) {
    s_prev = a.regime_in[src];
    if (s_prev < 0 || s_prev >= M) good = false, s_prev = 0;
  }
  if (!good) {
    raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    const double nan = Num<double>::nan();
    a.regime_out[n] = 0;
    a.log_weight[n] = nan;
    for (int i = 0; i < D; ++i) a.mean_out[n * D + i] = nan;
    for (int e = 0; e < TD; ++e) a.cov_out[n * TD + e] = nan;
    return;
  }
  const double u = a.uniforms[n];
  const double *row = a.particle_cdf != nullptr ? a.particle_cdf + src * M : cdf + (later ? s_prev * M : 0);
  int s = 0;
  for (int i = 0; i < M - 1; ++i) s += row[i] <= u ? 1 : 0;
  if (a.pinned_regime != nullptr && k == (int64_t)a.K - 1) {      // K38: the pinned slot takes the reference's regime
    s = a.pinned_regime[b];
    if (s < 0 || s >= M) {      // (as a stored regime outside [0, M))
      raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
      const double nan = Num<double>::nan();
      a.regime_out[n] = 0;
      a.log_weight[n] = nan;
      for (int i = 0; i < D; ++i) a.mean_out[n * D + i] = nan;
      for (int e = 0; e < TD; ++e) a.cov_out[n * TD + e] = nan;
      return;
    }
  }

  const double *Am = mdl + s * kPer, *bv = Am + DP * DP, *q2 = bv + DP, *Cm = q2 + DP, *dv = Cm + DYP * DP, *r2 = dv + DYP;

  // ---- predict -----------------------------------------------------------------------------------------------------------
  double mp[DP];
  SkCov<TP, sk_cov_in_lds(DP)> Pm;
  Pm.lds = mdl + M * kPer + threadIdx.x;
  if (later) {
    double mi[DP], Pi[TP];
    const double *mrow = a.mean_in + src * D, *prow = a.cov_in + src * TD;
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
    // P-_ij = A_i . W_j (P is symmetric): row i of A alone again, and the rows of W already there
#pragma unroll
    for (int i = 0; i < DP; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double acc = i == j ? q2[i] : 0.0;
#pragma unroll
        for (int l = 0; l < DP; ++l) acc = __builtin_fma(Am[i * DP + l], W[j][l], acc);
        Pm.set(sk_tri(i, j), acc);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      mp[i] = i < D ? a.m0[i] : 0.0;
      const double s0 = i < D ? a.s0[i] : 0.0;
#pragma unroll
      for (int j = 0; j <= i; ++j) Pm.set(sk_tri(i, j), i == j ? s0 * s0 : 0.0);
    }
  }

  // ---- innovation, U = C P-, S_ij = C_i . U_j + diag(r^2): row i of C alone serves e_i, U_i and S_i ---------------------------
  SK_REREAD_LDS();
  double e[DYP], U[DYP][DP], S[TY], yv[DYP];
  bool ob[DYP];
  int n_obs = Dy;
  if constexpr (Masked) {
    const uint8_t *orow = a.observed + b * Dy;
    n_obs = 0;
#pragma unroll
    for (int i = 0; i < DYP; ++i) {
      ob[i] = i < Dy ? orow[i] != 0 : false;
      n_obs += ob[i] ? 1 : 0;
    }
  } else {
#pragma unroll
    for (int i = 0; i < DYP; ++i) ob[i] = true;
  }
  if (a.y_is_float) {
    const float *yrow = (const float *)a.y + b * Dy;
#pragma unroll
    for (int i = 0; i < DYP; ++i) yv[i] = i < Dy ? (double)yrow[i] : 0.0;
  } else {
    const double *yrow = (const double *)a.y + b * Dy;
#pragma unroll
    for (int i = 0; i < DYP; ++i) yv[i] = i < Dy ? yrow[i] : 0.0;
  }
  if constexpr (Masked) {
#pragma unroll
    for (int i = 0; i < DYP; ++i) yv[i] = ob[i] ? yv[i] : 0.0;      // (may be NaN or Inf where not observed)
  }
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    if (i) SK_REREAD_LDS();
    double acc = yv[i] - dv[i];
#pragma unroll
    for (int l = 0; l < DP; ++l) acc = __builtin_fma(-Cm[i * DP + l], mp[l], acc);
    e[i] = Masked && !ob[i] ? 0.0 : acc;      // (a select: a non-finite y at an unobserved position ends here)
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double w = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) w = __builtin_fma(Cm[i * DP + c], Pm.get(sk_tri(c, l)), w);
      U[i][l] = Masked && !ob[i] ? 0.0 : w;
    }
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double w = i == j ? r2[i] : 0.0;
#pragma unroll
      for (int l = 0; l < DP; ++l) w = __builtin_fma(Cm[i * DP + l], U[j][l], w);
      S[sk_tri(i, j)] = Masked && !(ob[i] && ob[j]) ? (i == j ? 1.0 : 0.0) : w;
    }
  }

  // ---- Lam = chol(S) in place, column by column; inv[j] = 1 / Lam_jj -------------------------------------------------------
  double inv[DYP], log_det = 0.0;
  bool positive = true;
#pragma unroll
  for (int j = 0; j < DYP; ++j) {
    double pivot = S[sk_tri(j, j)];
#pragma unroll
    for (int c = 0; c < j; ++c) pivot = __builtin_fma(-S[sk_tri(j, c)], S[sk_tri(j, c)], pivot);
    positive = positive && pivot > 0.0;
    const double ljj = __builtin_sqrt(pivot);
    S[sk_tri(j, j)] = ljj;
    inv[j] = 1.0 / ljj;
    log_det += ::log(ljj);
#pragma unroll
    for (int i = j + 1; i < DYP; ++i) {
      double acc = S[sk_tri(i, j)];
#pragma unroll
      for (int c = 0; c < j; ++c) acc = __builtin_fma(-S[sk_tri(i, c)], S[sk_tri(j, c)], acc);
      S[sk_tri(i, j)] = acc * inv[j];
    }
  }

  // ---- v = Lam^-1 e, V = Lam^-1 U (in place) -------------------------------------------------------------------------------
  double quad = 0.0;
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    double acc = e[i];
#pragma unroll
    for (int c = 0; c < i; ++c) acc = __builtin_fma(-S[sk_tri(i, c)], e[c], acc);
    e[i] = acc * inv[i];
    quad = __builtin_fma(e[i], e[i], quad);
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double w = U[i][l];
#pragma unroll
      for (int c = 0; c < i; ++c) w = __builtin_fma(-S[sk_tri(i, c)], U[c][l], w);
      U[i][l] = w * inv[i];
    }
  }

  // ---- outputs -----------------------------------------------------------------------------------------------------------
  a.regime_out[n] = s;
  double *mout = a.mean_out + n * D, *pout = a.cov_out + n * TD;
  if (!positive) {
    const double nan = Num<double>::nan();
    a.log_weight[n] = nan;
    for (int i = 0; i < D; ++i) mout[i] = nan;
    for (int c = 0; c < TD; ++c) pout[c] = nan;
    return;
  }
  a.log_weight[n] = (-0.5 * quad - log_det) - (double)n_obs * kHalfLog2Pi;
#pragma unroll
  for (int l = 0; l < DP; ++l) {
    SK_REREAD_LDS();      // (row by row: neither the reads of P- nor the stores move across)
    double acc = mp[l];
#pragma unroll
    for (int i = 0; i < DYP; ++i) acc = __builtin_fma(U[i][l], e[i], acc);
    if (l < D) mout[l] = acc;
#pragma unroll
    for (int j = 0; j <= l; ++j) {
      double w = Pm.get(sk_tri(l, j));
#pragma unroll
      for (int i = 0; i < DYP; ++i) w = __builtin_fma(-U[i][l], U[i][j], w);
      if (l < D) pout[sk_tri(l, j)] = w;
    }
  }
}

}  // namespace aesmc

extern "C" int64_t aesmc_switching_max_latent_dim(void) { return aesmc::kSkMaxDim; }
extern "C" int64_t aesmc_switching_max_observation_dim(void) { return aesmc::kSkMaxDim; }
extern "C" int64_t aesmc_switching_max_regimes(void) { return aesmc::kSkMaxRegimes; }

namespace aesmc {

// K31 (particle_cdf NULL, `draw` false), K33 (`draw`: the regime from particle_cdf [B,K,M], the model's own cumulative
// rows not read) and K38 (`pinned`: pinned_regime [B] given): one set of checks, one launch.  K39 (`masked`: observed [B,Dy]
// given) is any of the three with the masked instantiation
static int sk_step(bool draw, bool pinned, bool masked, const uint8_t *observed, int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                   const double *mean_in, const double *cov_in, const int64_t *idx, const double *uniforms,
                   const double *particle_cdf, const int32_t *pinned_regime, const void *y, int32_t *regime_out,
                   double *mean_out, double *cov_out, double *log_weight, int32_t *flags, int64_t B, int64_t K,
                   void *stream) {
  if (draw && (particle_cdf == nullptr || !sk_aligned(particle_cdf, 8) ||
               sk_among(particle_cdf, {mean_out, cov_out, log_weight})))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (pinned && (pinned_regime == nullptr || !sk_aligned(pinned_regime, 4) || pinned_regime == regime_out))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (masked && (observed == nullptr || sk_among(observed, {regime_out, mean_out, cov_out, log_weight})))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (model == nullptr || uniforms == nullptr || regime_out == nullptr || mean_out == nullptr || cov_out == nullptr ||
      log_weight == nullptr || B < 0 || K < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool later = regime_in != nullptr;
  if (later != (mean_in != nullptr) || later != (cov_in != nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  const double *rows = later ? model->cdf : model->cdf0;
  if (!draw && (rows == nullptr || !sk_aligned(rows, 8))) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_observation(y, y_dtype) || !sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, true))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(regime_in, 4) || !sk_aligned(mean_in, 8) || !sk_aligned(cov_in, 8) || !sk_aligned(idx, 8) ||
      !sk_aligned(uniforms, 8) || !sk_aligned(regime_out, 4) || !sk_aligned(mean_out, 8) || !sk_aligned(cov_out, 8) ||
      !sk_aligned(log_weight, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (later && (regime_out == regime_in || mean_out == mean_in || cov_out == cov_in)) return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (!sk_extents_supported(model->M, model->D, model->Dy) || !sk_fits_32bit(B, K, kSkTriMax)) return AESMC_ERR_UNSUPPORTED;
  SwitchingArgs a;
  sk_fill_model(a, model);
  a.cdf = draw ? nullptr : rows;
  a.particle_cdf = draw ? particle_cdf : nullptr;
  a.pinned_regime = pinned ? pinned_regime : nullptr;
  a.m0 = model->m0, a.s0 = model->s0;
  a.regime_in = regime_in, a.mean_in = mean_in, a.cov_in = cov_in;
  a.idx = idx, a.uniforms = uniforms, a.y = y;
  a.observed = masked ? observed : nullptr;
  a.regime_out = regime_out, a.mean_out = mean_out, a.cov_out = cov_out, a.log_weight = log_weight;
  a.flags = flags;
  a.N = B * K, a.K = (uint32_t)K;
  a.y_is_float = y_dtype == AESMC_F32;
  const int dp = sk_pad(model->D), dyp = sk_pad(model->Dy);
  const size_t lds = ((draw ? 0 : later ? (size_t)a.M * a.M : (size_t)a.M) + (size_t)a.M * sk_per_regime(dp, dyp) +
                      (sk_cov_in_lds(dp) ? dp * (dp + 1) / 2 * kSkBlock : 0)) * sizeof(double);
  return sk_for_extents(dp, dyp, [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      return sk_launch(&switching_kalman_kernel<decltype(d)::value, decltype(dy)::value, decltype(m)::value>, sk_grid(a.N),
                       dim3(kSkBlock), lds, (hipStream_t)stream, a);
    });
  });
}

}  // namespace aesmc

extern "C" int aesmc_switching_kalman_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                           const double *mean_in, const double *cov_in, const int64_t *idx,
                                           const double *uniforms, const void *y, int32_t *regime_out, double *mean_out,
                                           double *cov_out, double *log_weight, int32_t *flags, int64_t B, int64_t K,
                                           void *stream) {
  return aesmc::sk_step(false, false, false, nullptr, y_dtype, model, regime_in, mean_in, cov_in, idx, uniforms, nullptr, nullptr, y,
                        regime_out, mean_out, cov_out, log_weight, flags, B, K, stream);
}

extern "C" int aesmc_switching_kalman_draw(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                           const double *mean_in, const double *cov_in, const int64_t *idx,
                                           const double *uniforms, const double *particle_cdf, const void *y,
                                           int32_t *regime_out, double *mean_out, double *cov_out, double *log_weight,
                                           int32_t *flags, int64_t B, int64_t K, void *stream) {
  return aesmc::sk_step(true, false, false, nullptr, y_dtype, model, regime_in, mean_in, cov_in, idx, uniforms, particle_cdf, nullptr, y,
                        regime_out, mean_out, cov_out, log_weight, flags, B, K, stream);
}

extern "C" int aesmc_switching_kalman_conditional_step(int y_dtype, const aesmc_switching_model *model,
                                                       const int32_t *regime_in, const double *mean_in, const double *cov_in,
                                                       const int64_t *idx, const double *uniforms,
                                                       const int32_t *pinned_regime, const void *y, int32_t *regime_out,
                                                       double *mean_out, double *cov_out, double *log_weight, int32_t *flags,
                                                       int64_t B, int64_t K, void *stream) {
  return aesmc::sk_step(false, true, false, nullptr, y_dtype, model, regime_in, mean_in, cov_in, idx, uniforms, nullptr, pinned_regime, y,
                        regime_out, mean_out, cov_out, log_weight, flags, B, K, stream);
}

// K49: K33's and K38's operands at once — every slot draws from its ancestor's row, slot K-1 takes the pinned regime
extern "C" int aesmc_switching_kalman_conditional_draw(int y_dtype, const aesmc_switching_model *model,
                                                       const int32_t *regime_in, const double *mean_in, const double *cov_in,
                                                       const int64_t *idx, const double *uniforms, const double *particle_cdf,
                                                       const int32_t *pinned_regime, const void *y, int32_t *regime_out,
                                                       double *mean_out, double *cov_out, double *log_weight, int32_t *flags,
                                                       int64_t B, int64_t K, void *stream) {
  return aesmc::sk_step(true, true, false, nullptr, y_dtype, model, regime_in, mean_in, cov_in, idx, uniforms, particle_cdf,
                        pinned_regime, y, regime_out, mean_out, cov_out, log_weight, flags, B, K, stream);
}

// K39: particle_cdf non-NULL is K33's form, pinned_regime non-NULL K38's, both NULL K31's (both given: K49's)
extern "C" int aesmc_switching_kalman_masked_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                                  const double *mean_in, const double *cov_in, const int64_t *idx,
                                                  const double *uniforms, const double *particle_cdf,
                                                  const int32_t *pinned_regime, const void *y, const uint8_t *observed,
                                                  int32_t *regime_out, double *mean_out, double *cov_out,
                                                  double *log_weight, int32_t *flags, int64_t B, int64_t K, void *stream) {
  return aesmc::sk_step(particle_cdf != nullptr, pinned_regime != nullptr, true, observed, y_dtype, model, regime_in, mean_in,
                        cov_in, idx, uniforms, particle_cdf, pinned_regime, y, regime_out, mean_out, cov_out, log_weight,
                        flags, B, K, stream);
}
