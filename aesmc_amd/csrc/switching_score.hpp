// The pair score of Rao-Blackwellised backward simulation, shared by the kernels that form it (switching_backward.hip: K35,
// a tile of trajectories per lane; switching_conditional.hip: K37, the one reference trajectory of a conditional sweep):
// the chains of K35's contract in include/aesmc_hip.h, in that order.
#pragma once
#include "switching_kalman.hpp"

namespace aesmc {

// F [TP] (F_ik, i >= k, at sk_tri(i, k)) and lam [DP] zero-padded to DP, in LDS; m, P the lane's particle; lp_at: where log
// Pi[s, s'] lies in LDS — read last, so that it occupies no register on the way; -inf gives -inf whatever the rest is; lw:
// the particle's log-weight, added when `weighted`.  Reads P through SK_REREAD_LDS once per row of W.
// The LDS operands are __restrict__ and hph is held where it is formed (below) for the compiler's sake alone: as a function
// the body is optimised once on its own before it is inlined, and without the two K35's 8-wide form took 283 registers where
// the same text in line took 174 (with them: 200, the same two wavefronts per SIMD, the same time: profiles/switching_gibbs.txt).
template <int DP, typename Cov>
__device__ __forceinline__ double switching_pair_score(const double *__restrict__ F, const double *__restrict__ lam,
                                                       const double (&m)[DP], const Cov &P,
                                                       const double *__restrict__ lp_at, double lw, bool weighted) {
  constexpr int TP = DP * (DP + 1) / 2;
  // ---- t = F^T m, h = lam - F t, the two quadratic terms in m ---------------------------------------------------------------
  double t[DP], h[DP], mq = 0.0, lm = 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int l = i; l < DP; ++l) acc = __builtin_fma(F[sk_tri(l, i)], m[l], acc);
    t[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < DP; ++i) mq = __builtin_fma(t[i], t[i], mq);
#pragma unroll
  for (int l = 0; l < DP; ++l) {
    double acc = lam[l];
#pragma unroll
    for (int i = 0; i <= l; ++i) acc = __builtin_fma(-F[sk_tri(l, i)], t[i], acc);
    h[l] = acc;
    lm = __builtin_fma(lam[l], m[l], lm);
  }
  // ---- h^T P h -----------------------------------------------------------------------------------------------------------------
  double hph = 0.0;
#pragma unroll
  for (int c = 0; c < DP; ++c) {
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < DP; ++l) acc = __builtin_fma(P.get(sk_tri(c, l)), h[l], acc);
    hph = __builtin_fma(h[c], acc, hph);
  }
  // hph is wanted only at the end: left alone, the compiler sinks its chain behind the last row of W and keeps the 36 values of
  // P it read for it alive across every row (72 registers at DP = 8).  This holds it here.
  asm volatile("" : "+v"(hph));
  // ---- W = Phi P row by row: row i gives v_i and row i of Lam = I + W Phi^T ------------------------------------------------------
  double v[DP], Lam[TP];
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    SK_REREAD_LDS();
    double W[DP];
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double acc = 0.0;
#pragma unroll
      for (int c = i; c < DP; ++c) acc = __builtin_fma(F[sk_tri(c, i)], P.get(sk_tri(c, l)), acc);
      W[l] = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < DP; ++l) acc = __builtin_fma(W[l], h[l], acc);
    v[i] = acc;
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double w = i == j ? 1.0 : 0.0;
#pragma unroll
      for (int l = j; l < DP; ++l) w = __builtin_fma(W[l], F[sk_tri(l, j)], w);
      Lam[sk_tri(i, j)] = w;
    }
  }
  // ---- G = chol(Lam) in place, x = G^-1 v in step ---------------------------------------------------------------------------------
  double inv[DP], log_det = 0.0;
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    double pivot = Lam[sk_tri(j, j)];
#pragma unroll
    for (int c = 0; c < j; ++c) pivot = __builtin_fma(-Lam[sk_tri(j, c)], Lam[sk_tri(j, c)], pivot);
    const double gjj = __builtin_sqrt(pivot);
    Lam[sk_tri(j, j)] = gjj;
    inv[j] = 1.0 / gjj;
    log_det += ::log(gjj);
#pragma unroll
    for (int i = j + 1; i < DP; ++i) {
      double acc = Lam[sk_tri(i, j)];
#pragma unroll
      for (int c = 0; c < j; ++c) acc = __builtin_fma(-Lam[sk_tri(i, c)], Lam[sk_tri(j, c)], acc);
      Lam[sk_tri(i, j)] = acc * inv[j];
    }
  }
  double xq = 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    double acc = v[i];
#pragma unroll
    for (int c = 0; c < i; ++c) acc = __builtin_fma(-Lam[sk_tri(i, c)], v[c], acc);
    v[i] = acc * inv[i];
    xq = __builtin_fma(v[i], v[i], xq);
  }
  // ---- the score ---------------------------------------------------------------------------------------------------------------
  const double lp = *lp_at;
  double score = weighted ? lw + lp : lp;
  score = score + lm;
  score = __builtin_fma(-0.5, mq, score);
  score = __builtin_fma(0.5, hph - xq, score);
  score = score - log_det;
  return lp == Num<double>::neg_inf() ? lp : score;
}

}  // namespace aesmc
