// The information step of Rao-Blackwellised backward simulation (Fong, Godsill, Doucet & West 2002; Whiteley, Andrieu &
// Doucet 2010; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016) for a switching linear-Gaussian state-space model —
// aesmc_switching_information_step (K34) of include/aesmc_hip.h.
//
// A backward trajectory carries, for its future regimes, p(y_{t+1..T-1} | z_t) = exp(c + lam^T z_t - 1/2 z_t^T Om z_t).  One
// launch, per trajectory, takes (Om, lam, c) of time t+1 to time t under the regime s'_{t+1}: the observation's information
// is added, the transition's noise integrated out (one D x D Cholesky factor of I + Q^1/2 Om Q^1/2, whose pivots are at
// least 1, and two forward substitutions), the result carried back through A, b, and the new Om factored once more — a
// Cholesky of a matrix that is only positive SEMI-definite, a pivot at or below 2^-40 of the largest diagonal entry giving a
// zero column — so that the pair scores (switching_backward.hip, K35) read the factor and never Om.
//
//   workgroup = 256 consecutive trajectories of the flattened [B N] range, one lane per trajectory;
//   model     staged once per workgroup into LDS by sk_stage_model (switching_kalman.hpp), as K31's: zero-padded to the
//             instantiation's extents DP, DYP (2, 4, 8 each), r^2 padded with ONE (its reciprocal 1, its logarithm 0);
//   chains    every value is ONE chain of float64 __builtin_fma in the header's order; a padded term multiplies a zero by a
//             zero.  The padded rows and columns of Om stay zero, their pivots are dropped by the rule above.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP,DYP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2,2>        58      0        0             8
//   <2,4>        60      0        0             8
//   <2,8>        62      0        0             8
//   <4,2>       110      0        0             4
//   <4,4>       118      0        0             4
//   <4,8>        98      0        0             4
//   <8,2>       256     74        0             1
//   <8,4>       256     76        0             1
//   <8,8>       256     74        0             1
// and of the masked instantiations (K41, aesmc_switching_masked_information_step):
//   <2,2>        57      0        0             8
//   <2,4>        72      0        0             7
//   <2,8>       112      0        0             4
//   <4,2>       108      0        0             4
//   <4,4>       102      0        0             4
//   <4,8>       158      0        0             3
//   <8,2>       256     78        0             1
//   <8,4>       256     74        0             1
//   <8,8>       256     74        0             1
// There are B N trajectories, not B N K pairs: this launch is a tenth of a step at N = 64, K = 1024 (profiles/
// switching_smoother.txt).  The 8-wide instantiations keep Oh, L and X (36 + 36 + 64 float64) live at once and move through
// the accumulation registers; none uses scratch, and they are not given K31's LDS layout.
#include "switching_host.hpp"

namespace aesmc {

struct InformationArgs {
  const double *A, *b, *q, *C, *d, *r;
  const int32_t *regime_next;                      // [B,N]
  const double *omega_in, *lambda_in, *c_in;       // all NULL: the zeros of the last step
  const void *y;                                   // [B,Dy]
  const uint8_t *observed;                         // K41: [B,Dy], nonzero = observed; NULL in the unmasked instantiations
  double *omega_out, *lambda_out, *c_out, *factor_out;
  int32_t *flags;
  int64_t total;                                   // B N
  uint32_t N;
  int M, D, Dy, y_is_float;
};

// Masked (K41): a component whose byte of `observed` is zero adds no information — its e and its 1 / r^2 are SELECTED to 0
// (its y is never read into a chain), its log r^2 is dropped, and the constant counts the observed components
template <int DP, int DYP, bool Masked>
__global__ __launch_bounds__(kSkBlock) void switching_information_kernel(const InformationArgs a) {
  extern __shared__ __attribute__((aligned(16))) double si_smem[];
  constexpr int kPer = sk_per_regime(DP, DYP);
  constexpr int TP = DP * (DP + 1) / 2;
  const int M = a.M, D = a.D, Dy = a.Dy;
  sk_stage_model<DP, DYP>(si_smem, M, D, Dy, a.A, a.b, a.q, a.C, a.d, a.r);
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (n >= a.total) return;
  const int64_t b = n / a.N;
  const int TD = D * (D + 1) / 2;
  double *om_out = a.omega_out + n * TD, *lam_out = a.lambda_out + n * D, *f_out = a.factor_out + n * TD;
  const int j = a.regime_next[n];
  if (j < 0 || j >= M) {
    raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    const double nan = Num<double>::nan();
    a.c_out[n] = nan;
    for (int i = 0; i < D; ++i) lam_out[i] = nan;
    for (int e = 0; e < TD; ++e) om_out[e] = nan, f_out[e] = nan;
    return;
  }
  const double *Am = si_smem + j * kPer, *bv = Am + DP * DP, *q2 = bv + DP, *Cm = q2 + DP, *dv = Cm + DYP * DP, *r2 = dv + DYP;

  double Oh[TP], lh[DP], c = 0.0;
  if (a.omega_in != nullptr) {
    const double *orow = a.omega_in + n * TD, *lrow = a.lambda_in + n * D;
#pragma unroll
    for (int e = 0; e < TP; ++e) Oh[e] = e < TD ? orow[e] : 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i) lh[i] = i < D ? lrow[i] : 0.0;
    c = a.c_in[n];
  } else {
#pragma unroll
    for (int e = 0; e < TP; ++e) Oh[e] = 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i) lh[i] = 0.0;
  }

  // ---- the observation: Oh = Om + C^T R^-1 C, lh = lam + C^T R^-1 (y - d), row i of C alone per round -------------------------
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
  bool seen[DYP];
  int n_obs = Dy;
  if constexpr (Masked) {
    const uint8_t *orow = a.observed + b * Dy;
    n_obs = 0;
#pragma unroll
    for (int i = 0; i < DYP; ++i) {
      seen[i] = i < Dy ? orow[i] != 0 : false;
      n_obs += seen[i] ? 1 : 0;
      yv[i] = seen[i] ? yv[i] : 0.0;      // (may be NaN or Inf where not observed)
    }
  } else {
#pragma unroll
    for (int i = 0; i < DYP; ++i) seen[i] = true;
  }
  double quad = 0.0, logr = 0.0;
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    if (i) SK_REREAD_LDS();
    const double e = Masked && !seen[i] ? 0.0 : yv[i] - dv[i];
    const double rho = Masked && !seen[i] ? 0.0 : 1.0 / r2[i];
    quad = __builtin_fma(e * rho, e, quad);
    logr += Masked && !seen[i] ? 0.0 : ::log(r2[i]);
    double G[DP];
#pragma unroll
    for (int l = 0; l < DP; ++l) G[l] = Cm[i * DP + l] * rho;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      lh[p] = __builtin_fma(G[p], e, lh[p]);
#pragma unroll
      for (int s = 0; s <= p; ++s) Oh[sk_tri(p, s)] = __builtin_fma(G[p], Cm[i * DP + s], Oh[sk_tri(p, s)]);
    }
  }
  double ch = __builtin_fma(-0.5, quad, c);
  ch = __builtin_fma(-0.5, logr, ch);
  ch = ch - (double)n_obs * kHalfLog2Pi;

  // ---- L = chol(I + Q^1/2 Oh Q^1/2) in place, column by column; inv[k] = 1 / L_kk -----------------------------------------------
  SK_REREAD_LDS();
  double sq[DP], L[TP], inv[DP], log_det = 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i) sq[i] = __builtin_sqrt(q2[i]);
#pragma unroll
  for (int p = 0; p < DP; ++p) {
#pragma unroll
    for (int s = 0; s <= p; ++s) L[sk_tri(p, s)] = __builtin_fma(sq[p] * sq[s], Oh[sk_tri(p, s)], p == s ? 1.0 : 0.0);
  }
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    double pivot = L[sk_tri(k, k)];
#pragma unroll
    for (int t = 0; t < k; ++t) pivot = __builtin_fma(-L[sk_tri(k, t)], L[sk_tri(k, t)], pivot);
    const double lkk = __builtin_sqrt(pivot);
    L[sk_tri(k, k)] = lkk;
    inv[k] = 1.0 / lkk;
    log_det += ::log(lkk);
#pragma unroll
    for (int i = k + 1; i < DP; ++i) {
      double acc = L[sk_tri(i, k)];
#pragma unroll
      for (int t = 0; t < k; ++t) acc = __builtin_fma(-L[sk_tri(i, t)], L[sk_tri(k, t)], acc);
      L[sk_tri(i, k)] = acc * inv[k];
    }
  }

  // ---- X = L^-1 (Q^1/2 Oh), w = L^-1 (Q^1/2 lh) ---------------------------------------------------------------------------------
  double X[DP][DP], w[DP], ww = 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    double acc = sq[i] * lh[i];
#pragma unroll
    for (int t = 0; t < i; ++t) acc = __builtin_fma(-L[sk_tri(i, t)], w[t], acc);
    w[i] = acc * inv[i];
    ww = __builtin_fma(w[i], w[i], ww);
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double x = sq[i] * Oh[sk_tri(i, l)];
#pragma unroll
      for (int t = 0; t < i; ++t) x = __builtin_fma(-L[sk_tri(i, t)], X[t][l], x);
      X[i][l] = x * inv[i];
    }
  }
  // ---- Ot = Oh - X^T X (in place), g = lh - X^T w (in place) -----------------------------------------------------------------------
#pragma unroll
  for (int p = 0; p < DP; ++p) {
#pragma unroll
    for (int i = 0; i < DP; ++i) lh[p] = __builtin_fma(-X[i][p], w[i], lh[p]);
#pragma unroll
    for (int s = 0; s <= p; ++s) {
      double acc = Oh[sk_tri(p, s)];
#pragma unroll
      for (int i = 0; i < DP; ++i) acc = __builtin_fma(-X[i][p], X[i][s], acc);
      Oh[sk_tri(p, s)] = acc;
    }
  }

  // ---- back through the transition: ob = Ot b, Om' = A^T Ot A, lam' = A^T (g - ob) -------------------------------------------------
  SK_REREAD_LDS();
  double ob[DP], gb[DP];
#pragma unroll
  for (int p = 0; p < DP; ++p) {
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < DP; ++l) acc = __builtin_fma(Oh[sk_tri(p, l)], bv[l], acc);
    ob[p] = acc;
    gb[p] = lh[p] - acc;
  }
  double cn = ch - log_det;
  cn = __builtin_fma(0.5, ww, cn);
#pragma unroll
  for (int i = 0; i < DP; ++i) cn = __builtin_fma(bv[i], lh[i], cn);
#pragma unroll
  for (int i = 0; i < DP; ++i) cn = __builtin_fma(-(0.5 * bv[i]), ob[i], cn);
  a.c_out[n] = cn;
#pragma unroll
  for (int i = 0; i < DP; ++i) {      // X is free: row i of Ot A
#pragma unroll
    for (int s = 0; s < DP; ++s) {
      double acc = 0.0;
#pragma unroll
      for (int t = 0; t < DP; ++t) acc = __builtin_fma(Oh[sk_tri(i, t)], Am[t * DP + s], acc);
      X[i][s] = acc;
    }
  }
  SK_REREAD_LDS();
  double F[TP];
#pragma unroll
  for (int p = 0; p < DP; ++p) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i) acc = __builtin_fma(Am[i * DP + p], gb[i], acc);
    if (p < D) lam_out[p] = acc;
#pragma unroll
    for (int s = 0; s <= p; ++s) {
      double o = 0.0;
#pragma unroll
      for (int i = 0; i < DP; ++i) o = __builtin_fma(Am[i * DP + p], X[i][s], o);
      F[sk_tri(p, s)] = o;
      if (p < D) om_out[sk_tri(p, s)] = o;
    }
  }

  // ---- the lower factor of Om', which is only positive semi-definite: a pivot at or below tau gives a zero column ----------------
  double top = F[0];
#pragma unroll
  for (int i = 1; i < DP; ++i) top = F[sk_tri(i, i)] > top ? F[sk_tri(i, i)] : top;
  const double tau = top * 0x1p-40;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    double pivot = F[sk_tri(k, k)];
#pragma unroll
    for (int t = 0; t < k; ++t) pivot = __builtin_fma(-F[sk_tri(k, t)], F[sk_tri(k, t)], pivot);
    const bool keep = pivot > tau;
    const double root = __builtin_sqrt(keep ? pivot : 1.0);
    const double rk = 1.0 / root;
    F[sk_tri(k, k)] = keep ? root : 0.0;
#pragma unroll
    for (int i = k + 1; i < DP; ++i) {
      double acc = F[sk_tri(i, k)];
#pragma unroll
      for (int t = 0; t < k; ++t) acc = __builtin_fma(-F[sk_tri(i, t)], F[sk_tri(k, t)], acc);
      F[sk_tri(i, k)] = keep ? acc * rk : 0.0;
    }
  }
#pragma unroll
  for (int e = 0; e < TP; ++e)
    if (e < TD) f_out[e] = F[e];
}

// K34, and K41 (`masked`: observed [B,Dy] given): one set of checks, one launch
static int si_step(bool masked, const uint8_t *observed, int y_dtype, const aesmc_switching_model *model,
                   const int32_t *regime_next, const double *omega_in, const double *lambda_in, const double *c_in,
                   const void *y, double *omega_out, double *lambda_out, double *c_out, double *factor_out, int32_t *flags,
                   int64_t B, int64_t N, void *stream) {
  if (masked && observed == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  if (model == nullptr || regime_next == nullptr || omega_out == nullptr || lambda_out == nullptr || c_out == nullptr ||
      factor_out == nullptr || B < 0 || N < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool later = omega_in != nullptr;
  if (later != (lambda_in != nullptr) || later != (c_in != nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_observation(y, y_dtype) || !sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, false))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(regime_next, 4) || !sk_aligned(omega_in, 8) || !sk_aligned(lambda_in, 8) || !sk_aligned(c_in, 8) ||
      !sk_aligned(omega_out, 8) || !sk_aligned(lambda_out, 8) || !sk_aligned(c_out, 8) || !sk_aligned(factor_out, 8) ||
      !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({omega_out, lambda_out, c_out, factor_out}, {regime_next, omega_in, lambda_in, c_in, y, observed}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0) return AESMC_OK;
  if (!sk_extents_supported(model->M, model->D, model->Dy) || !sk_fits_32bit(B, N, kSkTriMax)) return AESMC_ERR_UNSUPPORTED;
  InformationArgs a;
  sk_fill_model(a, model);
  a.regime_next = regime_next;
  a.omega_in = omega_in, a.lambda_in = lambda_in, a.c_in = c_in, a.y = y;
  a.observed = masked ? observed : nullptr;
  a.omega_out = omega_out, a.lambda_out = lambda_out, a.c_out = c_out, a.factor_out = factor_out;
  a.flags = flags;
  a.total = B * N, a.N = (uint32_t)N;
  a.y_is_float = y_dtype == AESMC_F32;
  const int dp = sk_pad(model->D), dyp = sk_pad(model->Dy);
  const size_t lds = (size_t)a.M * sk_per_regime(dp, dyp) * sizeof(double);      // (at most 20 KB: the limit is never raised)
  return sk_for_extents(dp, dyp, [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      return sk_launch(&switching_information_kernel<decltype(d)::value, decltype(dy)::value, decltype(m)::value>,
                       sk_grid(a.total), dim3(kSkBlock), lds, (hipStream_t)stream, a);
    });
  });
}

}  // namespace aesmc

extern "C" int aesmc_switching_information_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_next,
                                                const double *omega_in, const double *lambda_in, const double *c_in,
                                                const void *y, double *omega_out, double *lambda_out, double *c_out,
                                                double *factor_out, int32_t *flags, int64_t B, int64_t N, void *stream) {
  return aesmc::si_step(false, nullptr, y_dtype, model, regime_next, omega_in, lambda_in, c_in, y, omega_out, lambda_out,
                        c_out, factor_out, flags, B, N, stream);
}

extern "C" int aesmc_switching_masked_information_step(int y_dtype, const aesmc_switching_model *model,
                                                       const int32_t *regime_next, const double *omega_in,
                                                       const double *lambda_in, const double *c_in, const void *y,
                                                       const uint8_t *observed, double *omega_out, double *lambda_out,
                                                       double *c_out, double *factor_out, int32_t *flags, int64_t B,
                                                       int64_t N, void *stream) {
  return aesmc::si_step(true, observed, y_dtype, model, regime_next, omega_in, lambda_in, c_in, y, omega_out, lambda_out,
                        c_out, factor_out, flags, B, N, stream);
}
