// The two-filter combination of the Rao-Blackwellised state smoother (Fong, Godsill, Doucet & West 2002; Lindsten, Bunch,
// Saerkkae, Schoen & Godsill 2016) for a switching linear-Gaussian state-space model — aesmc_switching_smooth_combine (K36) of
// include/aesmc_hip.h.
//
// Given a regime trajectory the model is linear-Gaussian.  At time t the trajectory has the conditional Kalman filter's
// N(m, P) = p(z_t | y_{0:t}, s_{0:t}) (K31 under a forced regime) and K34's p(y_{t+1:T-1} | z_t, s_{t+1:T-1}) proportional to
// exp(lam^T z - 1/2 z^T Om z), Om = F F^T.  Their product is the smoothed N(m^s, P^s): with W = F^T P and Lam = I + W F
// (pivots at least 1, as K35's: no pivot test, P = 0 and q = 0 are fine, no predicted covariance is inverted),
// P^s = P - W^T Lam^-1 W and m^s = m + P^s (lam - Om m).  The lag-one cross-covariance Cov(z_{t+1}, z_t | y, s) is the
// off-diagonal block of (Sigma^-1 + diag(0, Oh))^-1 for the joint Sigma of (z_t, z_{t+1}) given y_{0:t}: with V = A P and
// Oh = Om_{t+1} + C^T R^-1 C (everything time t+1 and later says about z_{t+1}), cross = V - P^s_{t+1} (Oh V).
//
//   workgroup = 256 consecutive trajectories of the flattened [B N] range, one lane per trajectory;
//   model     read only for the cross-covariance: staged once per workgroup into LDS by sk_stage_model (switching_kalman.hpp)
//             as K34's, zero-padded to DP, DYP (2, 4, 8 each), r^2 padded with ONE; without cross_out nothing is staged;
//   phases    (1) the smoothed moments, row by row: row i of W gives row i of Lam, of its factor G and of U = G^-1 W, so one
//             row of W is live and Lam is never stored (every element is the header's chain; only the schedule is by rows);
//             (2) the cross-covariance, column by column: column l of V, of Oh V and of the result, 3 DP values live beside
//             Oh and P^s_{t+1}.  Phase 2 starts when F, G and U are dead and reuses their registers;
//   chains    every value is ONE chain of float64 __builtin_fma in the header's order; the triangular sums skip the
//             structural zeros of F, a padded term multiplies a zero by a zero.
//
// aesmc_switching_masked_smooth_combine (K42) is the kernel's second instantiation per extent (`Masked`): the observation of
// time t+1 enters Oh only through the components batch row b observed — 1 / r_i^2 is SELECTED to 0 elsewhere, K41's rule
// (switching_information.hip).  Nothing else of the combination knows about observations.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP,DYP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2,2>        54      0        0             8
//   <2,4>        54      0        0             8
//   <2,8>        54      0        0             8
//   <4,2>       131      0        0             3
//   <4,4>       131      0        0             3
//   <4,8>       131      0        0             3
//   <8,2>       256    138        0             1       P in LDS
//   <8,4>       256    134        0             1       P in LDS
//   <8,8>       256    134        0             1       P in LDS
// and of the masked instantiations (K42):
//   <2,2>        56      0        0             8
//   <2,4>        56      0        0             8
//   <2,8>        76      0        0             6
//   <4,2>       133      0        0             3
//   <4,4>       133      0        0             3
//   <4,8>       146      0        0             3
//   <8,2>       256    138        0             1       P in LDS
//   <8,4>       256    136        0             1       P in LDS
//   <8,8>       256    134        0             1       P in LDS
// The 8-wide instantiations hold F, G and U (36 + 36 + 64 float64) at once in phase 1, K34's footprint; P beside them would
// not fit, so they keep P in LDS in K31's [element][lane] layout (SkCov: 72 KB per workgroup beside the model's 20 KB at
// most) — the layout the siblings already use, chosen over a second kernel for the cross-covariance because phase 2 needs
// the same P again and is the lighter phase.  No instantiation uses scratch.
#include "switching_host.hpp"

namespace aesmc {

struct SmoothArgs {
  const double *A, *b, *q, *C, *d, *r;             // read with cross_out only
  const int32_t *regime_next;                      // [B,N], with cross_out only
  const double *mean, *cov, *factor, *lambda;      // [B,N,D], [B,N,D(D+1)/2], [B,N,D(D+1)/2], [B,N,D]
  const double *omega_next, *cov_next;             // [B,N,D(D+1)/2] each, with cross_out only; omega_next NULL: zeros
  double *mean_out, *cov_out, *cross_out;          // cross_out [B,N,D,D] or NULL
  int32_t *flags;
  int64_t total;                                   // B N
  int M, D, Dy;
  uint32_t N;                                      // K42 only: the row of a trajectory
  const uint8_t *observed_next;                    // K42: [B,Dy] of time t+1, nonzero = observed; NULL in the unmasked instantiations
};

// LDS: the staged model (with cross_out), then, for DP == 8, [TP][256] covariances
template <int DP, int DYP, bool Masked>
__global__ __launch_bounds__(kSkBlock) void switching_smooth_kernel(const SmoothArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ss_smem[];
  constexpr int kPer = sk_per_regime(DP, DYP);
  constexpr int TP = DP * (DP + 1) / 2;
  const int M = a.M, D = a.D, Dy = a.Dy;
  const bool cross = a.cross_out != nullptr;
  if (cross) {
    sk_stage_model<DP, DYP>(ss_smem, M, D, Dy, a.A, a.b, a.q, a.C, a.d, a.r);
    __syncthreads();
  }
  const int64_t n = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (n >= a.total) return;
  const int TD = D * (D + 1) / 2;
  double *m_out = a.mean_out + n * D, *p_out = a.cov_out + n * TD;
  int j = 0;
  if (cross) {
    j = a.regime_next[n];
    if (j < 0 || j >= M) {
      raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
      const double nan = Num<double>::nan();
      double *x_out = a.cross_out + n * D * D;
      for (int i = 0; i < D; ++i) m_out[i] = nan;
      for (int e = 0; e < TD; ++e) p_out[e] = nan;
      for (int e = 0; e < D * D; ++e) x_out[e] = nan;
      return;
    }
  }

  double m[DP], h[DP], F[TP];      // F_ik, i >= k, at sk_tri(i, k)
  SkCov<TP, sk_cov_in_lds(DP)> P;
  P.lds = ss_smem + (cross ? M * kPer : 0) + threadIdx.x;
  {
    const double *mrow = a.mean + n * D, *prow = a.cov + n * TD, *frow = a.factor + n * TD, *lrow = a.lambda + n * D;
#pragma unroll
    for (int i = 0; i < DP; ++i) m[i] = i < D ? mrow[i] : 0.0, h[i] = i < D ? lrow[i] : 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) F[e] = e < TD ? frow[e] : 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) P.set(e, e < TD ? prow[e] : 0.0);
  }

  // ---- t = F^T m, h = lam - F t ---------------------------------------------------------------------------------------------------
  {
    double t[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int l = i; l < DP; ++l) acc = __builtin_fma(F[sk_tri(l, i)], m[l], acc);
      t[i] = acc;
    }
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double acc = h[l];
#pragma unroll
      for (int i = 0; i <= l; ++i) acc = __builtin_fma(-F[sk_tri(l, i)], t[i], acc);
      h[l] = acc;
    }
  }

  // ---- row i of W = F^T P, of Lam = I + W F, of G = chol(Lam) and of U = G^-1 W ---------------------------------------------------
  double G[TP], inv[DP], U[DP][DP];
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    double W[DP];
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double acc = 0.0;
#pragma unroll
      for (int c = i; c < DP; ++c) acc = __builtin_fma(F[sk_tri(c, i)], P.get(sk_tri(c, l)), acc);
      W[l] = acc;
    }
#pragma unroll
    for (int k = 0; k <= i; ++k) {
      double w = i == k ? 1.0 : 0.0;
#pragma unroll
      for (int l = k; l < DP; ++l) w = __builtin_fma(W[l], F[sk_tri(l, k)], w);      // Lam_ik
#pragma unroll
      for (int c = 0; c < k; ++c) w = __builtin_fma(-G[sk_tri(i, c)], G[sk_tri(k, c)], w);
      if (k < i) {
        G[sk_tri(i, k)] = w * inv[k];
      } else {
        const double gii = __builtin_sqrt(w);
        G[sk_tri(i, i)] = gii;
        inv[i] = 1.0 / gii;
      }
    }
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double acc = W[l];
#pragma unroll
      for (int c = 0; c < i; ++c) acc = __builtin_fma(-G[sk_tri(i, c)], U[c][l], acc);
      U[i][l] = acc * inv[i];
    }
  }

  // ---- P^s = P - U^T U, m^s = m + P^s h -------------------------------------------------------------------------------------------
  {
    double S[TP];
#pragma unroll
    for (int p = 0; p < DP; ++p) {
#pragma unroll
      for (int s = 0; s <= p; ++s) {
        double acc = P.get(sk_tri(p, s));
#pragma unroll
        for (int i = 0; i < DP; ++i) acc = __builtin_fma(-U[i][p], U[i][s], acc);
        S[sk_tri(p, s)] = acc;
        if (p < D) p_out[sk_tri(p, s)] = acc;
      }
    }
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      double acc = m[p];
#pragma unroll
      for (int l = 0; l < DP; ++l) acc = __builtin_fma(S[sk_tri(p, l)], h[l], acc);
      if (p < D) m_out[p] = acc;
    }
  }
  if (!cross) return;

  // ---- Oh = Om_{t+1} + C^T R^-1 C, row i of C alone per round (K34's chains) ---------------------------------------------------------
  const double *Am = ss_smem + j * kPer, *Cm = Am + DP * DP + 2 * DP, *r2 = Cm + DYP * DP + DYP;
  double Oh[TP], Sn[TP];
  {
    const double *srow = a.cov_next + n * TD;
#pragma unroll
    for (int e = 0; e < TP; ++e) Sn[e] = e < TD ? srow[e] : 0.0;
  }
  if (a.omega_next != nullptr) {
    const double *orow = a.omega_next + n * TD;
#pragma unroll
    for (int e = 0; e < TP; ++e) Oh[e] = e < TD ? orow[e] : 0.0;
  } else {
#pragma unroll
    for (int e = 0; e < TP; ++e) Oh[e] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    if (i) SK_REREAD_LDS();
    double rho = 1.0 / r2[i];
    if constexpr (Masked) rho = (i < Dy && a.observed_next[(n / a.N) * Dy + i] != 0) ? rho : 0.0;
    double Gc[DP];
#pragma unroll
    for (int l = 0; l < DP; ++l) Gc[l] = Cm[i * DP + l] * rho;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
#pragma unroll
      for (int s = 0; s <= p; ++s) Oh[sk_tri(p, s)] = __builtin_fma(Gc[p], Cm[i * DP + s], Oh[sk_tri(p, s)]);
    }
  }

  // ---- column l of V = A P, of Y = Oh V and of cross = V - P^s_{t+1} Y ----------------------------------------------------------------
  double *x_out = a.cross_out + n * D * D;
#pragma unroll
  for (int l = 0; l < DP; ++l) {
    SK_REREAD_LDS();
    double V[DP], Y[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) acc = __builtin_fma(Am[i * DP + c], P.get(sk_tri(c, l)), acc);
      V[i] = acc;
    }
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      double acc = 0.0;
#pragma unroll
      for (int s = 0; s < DP; ++s) acc = __builtin_fma(Oh[sk_tri(p, s)], V[s], acc);
      Y[p] = acc;
    }
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      double acc = V[i];
#pragma unroll
      for (int p = 0; p < DP; ++p) acc = __builtin_fma(-Sn[sk_tri(i, p)], Y[p], acc);
      if (i < D && l < D) x_out[i * D + l] = acc;
    }
  }
}

// K36, and K42 (`masked`: observed_next [B,Dy] given, which only the cross-covariance reads): one set of checks, one launch
static int ss_combine(bool masked, const uint8_t *observed_next, const aesmc_switching_model *model,
                      const int32_t *regime_next, const double *mean, const double *cov, const double *factor,
                      const double *lambda, const double *omega_next, const double *cov_next, double *mean_out,
                      double *cov_out, double *cross_out, int32_t *flags, int64_t B, int64_t N, int64_t D, void *stream) {
  if (masked && (observed_next == nullptr || cross_out == nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (mean == nullptr || cov == nullptr || factor == nullptr || lambda == nullptr || mean_out == nullptr ||
      cov_out == nullptr || B < 0 || N < 0 || D < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool cross = cross_out != nullptr;
  if (cross) {
    if (model == nullptr || regime_next == nullptr || cov_next == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
    if (model->D != D || !sk_extents_positive(model->M, D, model->Dy) || !sk_model_operands(model, false))
      return AESMC_ERR_INVALID_ARGUMENT;
  } else if (model != nullptr || regime_next != nullptr || omega_next != nullptr || cov_next != nullptr) {
    return AESMC_ERR_INVALID_ARGUMENT;      // (what only the cross-covariance reads, given without asking for it)
  }
  if (!sk_aligned(regime_next, 4) || !sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(factor, 8) ||
      !sk_aligned(lambda, 8) || !sk_aligned(omega_next, 8) || !sk_aligned(cov_next, 8) || !sk_aligned(mean_out, 8) ||
      !sk_aligned(cov_out, 8) || !sk_aligned(cross_out, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({mean_out, cov_out, cross_out},
                           {regime_next, mean, cov, factor, lambda, omega_next, cov_next, observed_next}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0) return AESMC_OK;
  if (!sk_extents_supported(cross ? model->M : 0, D, cross ? model->Dy : 0) || !sk_fits_32bit(B, N, kSkMaxDim * kSkMaxDim))
    return AESMC_ERR_UNSUPPORTED;
  SmoothArgs a;
  a.A = a.b = a.q = a.C = a.d = a.r = nullptr;
  a.M = 0, a.Dy = 0, a.D = (int)D;
  if (cross) sk_fill_model(a, model);
  a.regime_next = regime_next;
  a.mean = mean, a.cov = cov, a.factor = factor, a.lambda = lambda, a.omega_next = omega_next, a.cov_next = cov_next;
  a.observed_next = masked ? observed_next : nullptr;
  a.mean_out = mean_out, a.cov_out = cov_out, a.cross_out = cross_out;
  a.flags = flags;
  a.total = B * N, a.N = (uint32_t)N;
  const int dp = sk_pad(D), dyp = cross ? sk_pad(model->Dy) : 2;      // (without cross_out nothing of extent Dy exists)
  const size_t lds = ((size_t)a.M * sk_per_regime(dp, dyp) + (sk_cov_in_lds(dp) ? (size_t)(dp * (dp + 1) / 2) * kSkBlock : 0)) *
                     sizeof(double);
  return sk_for_extents(dp, dyp, [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      return sk_launch(&switching_smooth_kernel<decltype(d)::value, decltype(dy)::value, decltype(m)::value>, sk_grid(a.total),
                       dim3(kSkBlock), lds, (hipStream_t)stream, a);
    });
  });
}

}  // namespace aesmc

extern "C" int aesmc_switching_smooth_combine(const aesmc_switching_model *model, const int32_t *regime_next,
                                              const double *mean, const double *cov, const double *factor,
                                              const double *lambda, const double *omega_next, const double *cov_next,
                                              double *mean_out, double *cov_out, double *cross_out, int32_t *flags,
                                              int64_t B, int64_t N, int64_t D, void *stream) {
  return aesmc::ss_combine(false, nullptr, model, regime_next, mean, cov, factor, lambda, omega_next, cov_next, mean_out,
                           cov_out, cross_out, flags, B, N, D, stream);
}

extern "C" int aesmc_switching_masked_smooth_combine(const aesmc_switching_model *model, const int32_t *regime_next,
                                                     const double *mean, const double *cov, const double *factor,
                                                     const double *lambda, const double *omega_next, const double *cov_next,
                                                     const uint8_t *observed_next, double *mean_out, double *cov_out,
                                                     double *cross_out, int32_t *flags, int64_t B, int64_t N, int64_t D,
                                                     void *stream) {
  return aesmc::ss_combine(true, observed_next, model, regime_next, mean, cov, factor, lambda, omega_next, cov_next, mean_out,
                           cov_out, cross_out, flags, B, N, D, stream);
}
