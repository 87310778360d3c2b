// The simulation smoother of the continuous state of a switching linear-Gaussian state-space model along GIVEN regime paths
// (Fruehwirth-Schnatter 1994; Carter & Kohn 1994: forward filtering, backward sampling) — aesmc_switching_state_draw (K47) of
// include/aesmc_hip.h: a draw z_{0:T-1} ~ p(z | s_{0:T-1}, y) per trajectory from the conditional Kalman filter's moments.
//
// The backward recursion is serial in time and independent across trajectories, so ONE launch does the whole pass: a lane owns
// a trajectory, keeps z_{t+1} in registers and walks t = T-1 .. 0.  A step, given z_{t+1} and j = s_{t+1}, is a Kalman
// measurement update of the filter's N(m_t, P_t) in which A_j, b_j, diag(q_j^2) play C, d, R and z_{t+1} plays y, then one
// affine draw (the header states the chains).  Both factorisations are of matrices that are only positive SEMI-definite (a
// q = 0 component, P = 0, the downdate of a state the next one determines) and follow K34's rule: a pivot at or below 2^-40 of
// the largest diagonal entry gives a zero column — for the first factor also a zero row of the two solves; for the second the
// threshold is taken from the INPUT covariance, so that what a downdate leaves of a determined direction is rounding, dropped.
//
//   workgroup = 256 consecutive trajectories of the flattened [B N] range, one lane per trajectory;
//   model     A, b, q^2 of every regime staged once per workgroup into LDS as float64, zero-padded to the instantiation's
//             extent DP (2, 4, 8) and read as broadcasts (C, d, r are not read: the filtered moments hold the observations);
//   prefetch  the lanes are few (B N) and each runs a long dependent float64 chain: the loads of step t-1 (m, P, the noise and
//             the regime at t) are issued before step t computes and consumed after it, pinned there by SK_REREAD_LDS;
//   chains    every value is ONE chain of float64 __builtin_fma in the header's order; a padded term multiplies a zero by a
//             zero, a padded pivot is 0 and dropped;
//   no atomics but the flag's: the same inputs give the same bits.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2>      76      0        0             6
//   <4>     166      0        0             3
//   <8>     256    154        0             1       P in LDS, two buffers
// The 8-wide instantiation holds V / U (64 float64) and a factor (36) at once; the current covariance and the prefetched one
// beside them would not fit, so it keeps both in LDS in K31's [element][lane] layout (SkCov: two buffers of 72 KB beside the
// model's 10 KB at most): the prefetched values pass through registers only while V = A P is formed.  No instantiation uses
// scratch.
#include "switching_host.hpp"

namespace aesmc {

struct StateDrawArgs {
  const double *A, *b, *q, *C, *d, *r;             // (C, d, r: sk_fill_model's, never read)
  const int32_t *regimes;                          // [T,B,N]
  const double *mean, *cov, *noise;                // [T,B,N,D], [T,B,N,D(D+1)/2], [T,B,N,D]
  const int32_t *regime_next;                      // [B,N] or NULL: the regime of time T
  const double *z_next;                            // [B,N,D] or NULL: the state of time T
  double *states;                                  // [T,B,N,D]
  int32_t *flags;
  int64_t total, T;                                // B N
  int M, D, Dy;
};

__host__ __device__ constexpr int sd_per_regime(int dp) { return dp * dp + 2 * dp; }      // A [DP,DP], b [DP], q^2 [DP]

// LDS: the staged A, b, q^2, then, for DP == 8, two [TP][256] covariance buffers
template <int DP> __global__ __launch_bounds__(kSkBlock) void switching_state_draw_kernel(const StateDrawArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sd_smem[];
  constexpr int kPer = sd_per_regime(DP);
  constexpr int TP = DP * (DP + 1) / 2;
  constexpr bool kLds = sk_cov_in_lds(DP);
  const int M = a.M, D = a.D;
  for (int e = threadIdx.x; e < M * kPer; e += kSkBlock) {
    const int s = e / kPer;
    int o = e - s * kPer;
    double v;
    if (o < DP * DP) {
      const int i = o / DP, l = o - i * DP;
      v = (i < D && l < D) ? a.A[(s * D + i) * D + l] : 0.0;
    } else if ((o -= DP * DP) < DP) {
      v = o < D ? a.b[s * D + o] : 0.0;
    } else {
      o -= DP;
      const double qv = o < D ? a.q[s * D + o] : 0.0;
      v = qv * qv;
    }
    sd_smem[e] = v;
  }
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (n >= a.total) return;      // (no barrier follows; a lane's covariance slots in LDS are its own)
  const int TD = D * (D + 1) / 2;
  const int64_t total = a.total;
  const double nan = Num<double>::nan();

  double m[DP], eps[DP], zn[DP];
  SkCov<TP, kLds> P;
  double *spare = sd_smem + M * kPer + threadIdx.x + TP * kSkBlock;      // (kLds: the buffer the next step's P is written to)
  P.lds = sd_smem + M * kPer + threadIdx.x;
  {
    const int64_t row = (a.T - 1) * total + n;
    const double *mrow = a.mean + row * D, *prow = a.cov + row * TD, *erow = a.noise + row * D;
#pragma unroll
    for (int i = 0; i < DP; ++i) m[i] = i < D ? mrow[i] : 0.0, eps[i] = i < D ? erow[i] : 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) P.set(e, e < TD ? prow[e] : 0.0);
  }
  bool have = a.regime_next != nullptr, dead = false;
  int j = 0;
#pragma unroll
  for (int i = 0; i < DP; ++i) zn[i] = 0.0;
  if (have) {
    j = a.regime_next[n];
    const double *zrow = a.z_next + n * D;
#pragma unroll
    for (int i = 0; i < DP; ++i) zn[i] = i < D ? zrow[i] : 0.0;
  }

  for (int64_t t = a.T - 1; t >= 0; --t) {
    // ---- step t-1's operands, on their way while step t computes ------------------------------------------------------------------
    const bool more = t > 0;
    double mN[DP], eN[DP], PN[TP];
    int jN = 0;
#pragma unroll
    for (int i = 0; i < DP; ++i) mN[i] = 0.0, eN[i] = 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) PN[e] = 0.0;
    if (more) {
      const int64_t row = (t - 1) * total + n;
      const double *mrow = a.mean + row * D, *prow = a.cov + row * TD, *erow = a.noise + row * D;
      jN = a.regimes[t * total + n];
#pragma unroll
      for (int i = 0; i < DP; ++i) mN[i] = i < D ? mrow[i] : 0.0, eN[i] = i < D ? erow[i] : 0.0;
#pragma unroll
      for (int e = 0; e < TP; ++e) PN[e] = e < TD ? prow[e] : 0.0;
    }
    SK_REREAD_LDS();

    double top = P.get(0);      // of the INPUT covariance: the second factor's threshold
#pragma unroll
    for (int i = 1; i < DP; ++i) top = P.get(sk_tri(i, i)) > top ? P.get(sk_tri(i, i)) : top;
    double Lp[TP];              // P', then its factor L'
    if (have) {
      if (j < 0 || j >= M) {
        raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
        dead = true;
        j = 0;
      }
      const double *Am = sd_smem + j * kPer, *bv = Am + DP * DP, *q2 = bv + DP;
      // ---- V = A P, e = (z_{t+1} - b) - A m ---------------------------------------------------------------------------------------
      double V[DP][DP], v[DP];
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        double acc = zn[i] - bv[i];
#pragma unroll
        for (int l = 0; l < DP; ++l) acc = __builtin_fma(-Am[i * DP + l], m[l], acc);
        v[i] = acc;
#pragma unroll
        for (int l = 0; l < DP; ++l) {
          double w = 0.0;
#pragma unroll
          for (int c = 0; c < DP; ++c) w = __builtin_fma(Am[i * DP + c], P.get(sk_tri(c, l)), w);
          V[i][l] = w;
        }
      }
      if constexpr (kLds) {
        if (more) {
#pragma unroll
          for (int e = 0; e < TP; ++e) spare[e * kSkBlock] = PN[e];
        }
      }
      SK_REREAD_LDS();
      // ---- S = A V^T + diag(q^2), its factor L in place (column by column), rk[k] = 1 / L_kk or 0 -------------------------------------
      double L[TP], rk[DP];
#pragma unroll
      for (int i = 0; i < DP; ++i) {
#pragma unroll
        for (int k = 0; k <= i; ++k) {
          double acc = i == k ? q2[i] : 0.0;
#pragma unroll
          for (int l = 0; l < DP; ++l) acc = __builtin_fma(Am[i * DP + l], V[k][l], acc);
          L[sk_tri(i, k)] = acc;
        }
      }
      double big = L[0];
#pragma unroll
      for (int i = 1; i < DP; ++i) big = L[sk_tri(i, i)] > big ? L[sk_tri(i, i)] : big;
      const double tau = big * 0x1p-40;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        double pivot = L[sk_tri(k, k)];
#pragma unroll
        for (int c = 0; c < k; ++c) pivot = __builtin_fma(-L[sk_tri(k, c)], L[sk_tri(k, c)], pivot);
        const bool keep = pivot > tau;
        const double root = __builtin_sqrt(keep ? pivot : 1.0);
        const double inv = 1.0 / root;
        rk[k] = keep ? inv : 0.0;
#pragma unroll
        for (int i = k + 1; i < DP; ++i) {
          double acc = L[sk_tri(i, k)];
#pragma unroll
          for (int c = 0; c < k; ++c) acc = __builtin_fma(-L[sk_tri(i, c)], L[sk_tri(k, c)], acc);
          L[sk_tri(i, k)] = keep ? acc * inv : 0.0;
        }
      }
      // ---- v = L^-1 e, U = L^-1 V (in place); a dropped pivot's row is zero -----------------------------------------------------------
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        const bool keep = rk[i] != 0.0;
        double acc = v[i];
#pragma unroll
        for (int c = 0; c < i; ++c) acc = __builtin_fma(-L[sk_tri(i, c)], v[c], acc);
        v[i] = keep ? acc * rk[i] : 0.0;
#pragma unroll
        for (int l = 0; l < DP; ++l) {
          double u = V[i][l];
#pragma unroll
          for (int c = 0; c < i; ++c) u = __builtin_fma(-L[sk_tri(i, c)], V[c][l], u);
          V[i][l] = keep ? u * rk[i] : 0.0;
        }
      }
      // ---- P' = P - U^T U, m' = m + U^T v ------------------------------------------------------------------------------------------------
#pragma unroll
      for (int p = 0; p < DP; ++p) {
#pragma unroll
        for (int s = 0; s <= p; ++s) {
          double acc = P.get(sk_tri(p, s));
#pragma unroll
          for (int i = 0; i < DP; ++i) acc = __builtin_fma(-V[i][p], V[i][s], acc);
          Lp[sk_tri(p, s)] = acc;
        }
        double acc = m[p];
#pragma unroll
        for (int i = 0; i < DP; ++i) acc = __builtin_fma(V[i][p], v[i], acc);
        m[p] = acc;
      }
    } else {
#pragma unroll
      for (int e = 0; e < TP; ++e) Lp[e] = P.get(e);
      if constexpr (kLds) {
        if (more) {
#pragma unroll
          for (int e = 0; e < TP; ++e) spare[e * kSkBlock] = PN[e];
        }
      }
    }

    // ---- L' = chol(P') under the input covariance's threshold, z_t = m' + L' eps ---------------------------------------------------------
    const double tau2 = top * 0x1p-40;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double pivot = Lp[sk_tri(k, k)];
#pragma unroll
      for (int c = 0; c < k; ++c) pivot = __builtin_fma(-Lp[sk_tri(k, c)], Lp[sk_tri(k, c)], pivot);
      const bool keep = pivot > tau2;
      const double root = __builtin_sqrt(keep ? pivot : 1.0);
      const double inv = 1.0 / root;
      Lp[sk_tri(k, k)] = keep ? root : 0.0;
#pragma unroll
      for (int i = k + 1; i < DP; ++i) {
        double acc = Lp[sk_tri(i, k)];
#pragma unroll
        for (int c = 0; c < k; ++c) acc = __builtin_fma(-Lp[sk_tri(i, c)], Lp[sk_tri(k, c)], acc);
        Lp[sk_tri(i, k)] = keep ? acc * inv : 0.0;
      }
    }
    double *zrow = a.states + (t * total + n) * D;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      double acc = m[p];
#pragma unroll
      for (int k = 0; k <= p; ++k) acc = __builtin_fma(Lp[sk_tri(p, k)], eps[k], acc);
      zn[p] = dead ? nan : acc;
      if (p < D) zrow[p] = zn[p];
    }

    // ---- step t-1's operands become the current ones ------------------------------------------------------------------------------------
    if (more) {
#pragma unroll
      for (int i = 0; i < DP; ++i) m[i] = mN[i], eps[i] = eN[i];
      if constexpr (kLds) {
        double *used = P.lds;
        P.lds = spare;
        spare = used;
      } else {
#pragma unroll
        for (int e = 0; e < TP; ++e) P.set(e, PN[e]);
      }
      j = jN;
      have = true;
    }
  }
}

}  // namespace aesmc

extern "C" int aesmc_switching_state_draw(const aesmc_switching_model *model, const int32_t *regimes, const double *mean,
                                          const double *cov, const double *noise, const int32_t *regime_next,
                                          const double *z_next, double *states, int32_t *flags, int64_t T, int64_t B,
                                          int64_t N, void *stream) {
  using namespace aesmc;
  if (model == nullptr || regimes == nullptr || mean == nullptr || cov == nullptr || noise == nullptr || states == nullptr ||
      T < 1 || B < 0 || N < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if ((regime_next != nullptr) != (z_next != nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, false)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(regimes, 4) || !sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(noise, 8) ||
      !sk_aligned(regime_next, 4) || !sk_aligned(z_next, 8) || !sk_aligned(states, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({states}, {regimes, mean, cov, noise, regime_next, z_next})) return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0) return AESMC_OK;
  if (!sk_extents_supported(model->M, model->D, model->Dy) || !sk_fits_32bit(B, N, kSkMaxDim * kSkMaxDim))
    return AESMC_ERR_UNSUPPORTED;
  StateDrawArgs a;
  sk_fill_model(a, model);
  a.regimes = regimes, a.mean = mean, a.cov = cov, a.noise = noise, a.regime_next = regime_next, a.z_next = z_next;
  a.states = states, a.flags = flags;
  a.total = B * N, a.T = T;
  const int dp = sk_pad(model->D);
  const size_t lds = ((size_t)a.M * sd_per_regime(dp) + (sk_cov_in_lds(dp) ? (size_t)2 * (dp * (dp + 1) / 2) * kSkBlock : 0)) *
                     sizeof(double);      // (at most 10 KB + 144 KB)
  return sk_for_extent(dp, [&](auto d) {
    return sk_launch(&switching_state_draw_kernel<decltype(d)::value>, sk_grid(a.total), dim3(kSkBlock), lds,
                     (hipStream_t)stream, a);
  });
}
