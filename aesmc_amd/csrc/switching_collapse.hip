// The two kernels of the collapsed-mixture filter and smoother of a switching linear-Gaussian state-space model (GPB2, which
// is Kim's filter — Kim 1994; Kim & Nelson 1999 — and its first-order cousin IMM, Blom & Bar-Shalom 1988):
// aesmc_switching_collapse (K50) and aesmc_switching_pair_smooth (K51) of include/aesmc_hip.h.  The filter carries M
// Gaussians per series, no particles and no random numbers; a step is K31 with the regime forced on M^2 (order 2) or M
// (order 1) slots, and what K31 lacks is here.
//
// K50  the moment-matching collapse of Gaussian mixtures: group (b,g) replaces its N weighted components by ONE Gaussian of
//      the same mass, mean and covariance.  One lane per group walks its components three times (the largest weight and the
//      normaliser, the mean, the centred covariance); the header states the chains.  `mean` and `cov` take an element stride
//      per group, 0 for components that every group of a batch row shares (IMM's mixing: one set of components, M weight rows).
//        workgroup = 256 consecutive groups of the flattened [B G] range; n is a run-time loop, p and s are unrolled over the
//        instantiation's extent DP (2, 4, 8) with the loads guarded by D.
// K51  a Rauch-Tung-Striebel step between mixture components: lane (b,i,j) smooths component i filtered at t against regime
//      j's smoothed component at t+1.  It is K47's measurement update (A_j, b_j, diag(q_j^2) as C, d, R; the smoothed mean
//      as y) with the smoothed covariance carried through the gain: P' = P - U^T U + U^T (L^-1 Ps L^-T) U.  Chains and the
//      pivot rule are K47's: a pivot of S at or below 2^-40 of its largest diagonal entry gives a zero row of every solve, so
//      q = 0 components and P = 0 are fine.
//        model     A, b, q^2 of every regime staged once per workgroup by sk_stage_model (its observation part has extent 0)
//                  and read as broadcasts;
//        registers U (DP^2) and the factor (DP (DP + 1) / 2) are live together with X = L^-1 Ps (DP^2) and both covariances:
//                  at DP == 8 that is past the register file, so that instantiation keeps P, Ps and X in LDS in K31's
//                  [element][lane] layout (SkCov) and runs 64 lanes per workgroup (136 values per lane: 68 KB beside the
//                  model's 10 KB at most).  The launch has only B M^2 lanes: occupancy does not matter.
//        Y = Gm U  is formed a column at a time, just before the column of P' that reads it.
// No atomics in either: the same inputs give the same bits.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950):
//   kernel  <DP>  lanes  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   K50     <2>    256     64      0        0             8
//   K50     <4>    256    100      0        0             4
//   K50     <8>    256    221      0        0             2
//   K51     <2>    256     59      0        0             8
//   K51     <4>    256    135      0        0             3
//   K51     <8>     64    256    106        0             1       P, Ps and X in LDS
// No instantiation uses scratch.  LDS is dynamic: K50 none; K51 the model's 8 M (DP^2 + 2 DP) bytes (at most 10 KB) and
// 68 KB more at DP == 8.
#include "switching_host.hpp"

namespace aesmc {

constexpr int kScMaxComponents = 256;      // N
constexpr int kScMaxGroups = 256;          // G

struct CollapseArgs {
  const double *mean, *cov, *log_weight;      // [B,G,N,D], [B,G,N,D(D+1)/2] by the group strides; [B,G,N]
  double *log_mass, *mean_out, *cov_out;      // [B,G], [B,G,D], [B,G,D(D+1)/2]
  int64_t mean_stride, cov_stride;            // elements between groups; 0: the row's N components are shared
  int64_t total;                              // B G
  int G, N, D;
};

template <int DP> __global__ __launch_bounds__(kSkBlock) void switching_collapse_kernel(const CollapseArgs a) {
  constexpr int TP = DP * (DP + 1) / 2;
  const int64_t lane = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (lane >= a.total) return;
  const int N = a.N, D = a.D, TD = D * (D + 1) / 2;
  const int64_t b = lane / a.G, g = lane - b * a.G;
  const double *lw = a.log_weight + lane * N;
  const double *mean = a.mean + b * (a.mean_stride ? a.G * a.mean_stride : (int64_t)N * D) + g * a.mean_stride;
  const double *cov = a.cov + b * (a.cov_stride ? a.G * a.cov_stride : (int64_t)N * TD) + g * a.cov_stride;
  double *mass_out = a.log_mass + lane, *mrow_out = a.mean_out + lane * D, *crow_out = a.cov_out + lane * TD;
  const double ninf = Num<double>::neg_inf();

  // ---- top = max_n lw_n; a NaN weight makes the group NaN, no finite weight makes it empty ----------------------------------------
  double top = ninf;
  bool bad = false;
  for (int n = 0; n < N; ++n) {
    const double w = lw[n];
    bad = bad || w != w;
    top = w > top ? w : top;
  }
  if (bad || top == ninf) {
    const double fill = bad ? Num<double>::nan() : 0.0;
    *mass_out = bad ? fill : ninf;
    for (int p = 0; p < D; ++p) mrow_out[p] = fill;
    for (int e = 0; e < TD; ++e) crow_out[e] = fill;
    return;
  }
  // ---- sum = 0 + sum_n exp(lw_n - top) -----------------------------------------------------------------------------------------------
  double sum = 0.0;
  for (int n = 0; n < N; ++n) sum = sum + exp(lw[n] - top);
  const double scale = 1.0 / sum;
  *mass_out = top + log(sum);
  // ---- mean_p = 0 + sum_n w_n m_np (a component of weight -inf is not read) ----------------------------------------------------------
  double m[DP];
#pragma unroll
  for (int p = 0; p < DP; ++p) m[p] = 0.0;
  for (int n = 0; n < N; ++n) {
    const double l = lw[n];
    if (l == ninf) continue;
    const double w = exp(l - top) * scale;
    const double *row = mean + (int64_t)n * D;
#pragma unroll
    for (int p = 0; p < DP; ++p) m[p] = __builtin_fma(w, p < D ? row[p] : 0.0, m[p]);
  }
  // ---- cov_ps = 0 + sum_n [w_n P_n,ps, then (w_n d_np) d_ns], d_n = m_n - mean ----------------------------------------------------
  double c[TP];
#pragma unroll
  for (int e = 0; e < TP; ++e) c[e] = 0.0;
  for (int n = 0; n < N; ++n) {
    const double l = lw[n];
    if (l == ninf) continue;
    const double w = exp(l - top) * scale;
    const double *row = mean + (int64_t)n * D, *prow = cov + (int64_t)n * TD;
    double d[DP];
#pragma unroll
    for (int p = 0; p < DP; ++p) d[p] = (p < D ? row[p] : 0.0) - m[p];
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      const double wd = w * d[p];
#pragma unroll
      for (int s = 0; s <= p; ++s) {
        const int e = sk_tri(p, s);
        c[e] = __builtin_fma(w, e < TD ? prow[e] : 0.0, c[e]);
        c[e] = __builtin_fma(wd, d[s], c[e]);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < DP; ++p)
    if (p < D) mrow_out[p] = m[p];
#pragma unroll
  for (int e = 0; e < TP; ++e)
    if (e < TD) crow_out[e] = c[e];
}

struct PairSmoothArgs {
  const double *A, *b, *q, *C, *d, *r;             // (C, d, r: sk_fill_model's, never read)
  const double *mean, *cov;                        // [B,M,D], [B,M,D(D+1)/2]: the components filtered at t
  const double *mean_next, *cov_next;              // the same shapes: the components smoothed at t+1
  double *mean_out, *cov_out;                      // [B,M,M,D], [B,M,M,D(D+1)/2]: (b, i, j)
  int64_t total;                                   // B M M
  int M, D, Dy;
};

__host__ __device__ constexpr int ps_lanes(int dp) { return sk_cov_in_lds(dp) ? 64 : kSkBlock; }
// LDS values per lane of the instantiations that keep P, Ps and X there
__host__ __device__ constexpr int ps_per_lane(int dp) { return sk_cov_in_lds(dp) ? dp * (dp + 1) + dp * dp : 0; }

// LDS: the staged A, b, q^2, then, for DP == 8, [TP][lanes] of P, [TP][lanes] of Ps and [DP DP][lanes] of X
template <int DP> __global__ __launch_bounds__(ps_lanes(DP)) void switching_pair_smooth_kernel(const PairSmoothArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ps_smem[];
  constexpr int kLanes = ps_lanes(DP);
  constexpr int kPer = sk_per_regime(DP, 0);
  constexpr int TP = DP * (DP + 1) / 2;
  constexpr bool kLds = sk_cov_in_lds(DP);
  const int M = a.M, D = a.D;
  sk_stage_model<DP, 0, kLanes>(ps_smem, M, D, 0, a.A, a.b, a.q, a.C, a.d, a.r);
  __syncthreads();
  const int64_t lane = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (lane >= a.total) return;      // (no barrier follows; a lane's slots in LDS are its own)
  const int TD = D * (D + 1) / 2;
  const int64_t pair = lane / M;      // b M + i
  const int j = (int)(lane - pair * M);
  const int64_t next = (pair / M) * M + j;      // b M + j

  double m[DP], v[DP];
  SkCov<TP, kLds, kLanes> P, Ps;
  SkCov<DP * DP, kLds, kLanes> X;
  P.lds = ps_smem + M * kPer + threadIdx.x;
  Ps.lds = P.lds + TP * kLanes;
  X.lds = Ps.lds + TP * kLanes;
  const double *Am = ps_smem + j * kPer, *bv = Am + DP * DP, *q2 = bv + DP;
  {
    const double *mrow = a.mean + pair * D, *prow = a.cov + pair * TD;
    const double *srow = a.mean_next + next * D, *qrow = a.cov_next + next * TD;
#pragma unroll
    for (int i = 0; i < DP; ++i) m[i] = i < D ? mrow[i] : 0.0, v[i] = i < D ? srow[i] : 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) P.set(e, e < TD ? prow[e] : 0.0), Ps.set(e, e < TD ? qrow[e] : 0.0);
  }
  SK_REREAD_LDS();
  // ---- V = A P, e = (ms - b) - A m ----------------------------------------------------------------------------------------------------
  double V[DP][DP];
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    double acc = v[i] - bv[i];
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
  SK_REREAD_LDS();
  // ---- S = A V^T + diag(q^2), its factor L in place (column by column), rk[k] = 1 / L_kk or 0 ----------------------------------------
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
  // ---- v = L^-1 e, U = L^-1 V (in place), X = L^-1 Ps; a dropped pivot's row is zero ------------------------------------------------
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
      double x = Ps.get(sk_tri(i, l));
#pragma unroll
      for (int c = 0; c < i; ++c) x = __builtin_fma(-L[sk_tri(i, c)], X.get(c * DP + l), x);
      X.set(i * DP + l, keep ? x * rk[i] : 0.0);
    }
  }
  SK_REREAD_LDS();
  // ---- Gm = X L^-T (in place, row by row: Gm_ik = (X_ik - sum_{c<k} Gm_ic L_kc) rk_k); a dropped pivot's column is zero ------------
#pragma unroll
  for (int i = 0; i < DP; ++i) {
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double acc = X.get(i * DP + k);
#pragma unroll
      for (int c = 0; c < k; ++c) acc = __builtin_fma(-X.get(i * DP + c), L[sk_tri(k, c)], acc);
      X.set(i * DP + k, rk[k] != 0.0 ? acc * rk[k] : 0.0);
    }
  }
  SK_REREAD_LDS();
  // ---- m' = m + U^T v;  Y = Gm U a column at a time;  P' = P - U^T U + U^T Y -----------------------------------------------------------
  double *mout = a.mean_out + lane * D, *cout = a.cov_out + lane * TD;
#pragma unroll
  for (int p = 0; p < DP; ++p) {
    double acc = m[p];
#pragma unroll
    for (int i = 0; i < DP; ++i) acc = __builtin_fma(V[i][p], v[i], acc);
    if (p < D) mout[p] = acc;
  }
#pragma unroll
  for (int s = 0; s < DP; ++s) {
    double Y[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) acc = __builtin_fma(X.get(k * DP + c), V[c][s], acc);
      Y[k] = acc;
    }
#pragma unroll
    for (int p = s; p < DP; ++p) {
      double acc = P.get(sk_tri(p, s));
#pragma unroll
      for (int k = 0; k < DP; ++k) acc = __builtin_fma(-V[k][p], V[k][s], acc);
#pragma unroll
      for (int k = 0; k < DP; ++k) acc = __builtin_fma(V[k][p], Y[k], acc);
      if (sk_tri(p, s) < TD) cout[sk_tri(p, s)] = acc;
    }
  }
}

}  // namespace aesmc

extern "C" int aesmc_switching_collapse(const double *mean, int64_t mean_group_stride, const double *cov,
                                        int64_t cov_group_stride, const double *log_weight, double *log_mass,
                                        double *mean_out, double *cov_out, int64_t B, int64_t G, int64_t N, int64_t D,
                                        void *stream) {
  using namespace aesmc;
  if (mean == nullptr || cov == nullptr || log_weight == nullptr || log_mass == nullptr || mean_out == nullptr ||
      cov_out == nullptr || B < 0 || G < 0 || N < 0 || D < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  // a group stride is 0 or the dense one (past 2^20 the extents are refused below whatever it is: no product is formed)
  const auto stride_fits = [&](int64_t stride, int64_t per) {
    if (stride == 0) return true;
    if (N > (1 << 20) || D > (1 << 20)) return stride > 0;
    return stride == N * per;
  };
  if (!stride_fits(mean_group_stride, D) || !stride_fits(cov_group_stride, D * (D + 1) / 2)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(log_weight, 8) || !sk_aligned(log_mass, 8) ||
      !sk_aligned(mean_out, 8) || !sk_aligned(cov_out, 8))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({log_mass, mean_out, cov_out}, {mean, cov, log_weight})) return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || G == 0) return AESMC_OK;
  if (D > kSkMaxDim || N > kScMaxComponents || G > kScMaxGroups || !sk_fits_32bit(B, G, 1)) return AESMC_ERR_UNSUPPORTED;
  CollapseArgs a;
  a.mean = mean, a.cov = cov, a.log_weight = log_weight, a.log_mass = log_mass, a.mean_out = mean_out, a.cov_out = cov_out;
  a.mean_stride = mean_group_stride, a.cov_stride = cov_group_stride;
  a.total = B * G, a.G = (int)G, a.N = (int)N, a.D = (int)D;
  return sk_for_extent(sk_pad(D), [&](auto d) {
    return sk_launch(&switching_collapse_kernel<decltype(d)::value>, sk_grid(a.total), dim3(kSkBlock), 0, (hipStream_t)stream,
                     a);
  });
}

extern "C" int aesmc_switching_pair_smooth(const aesmc_switching_model *model, const double *mean, const double *cov,
                                           const double *mean_next, const double *cov_next, double *mean_out,
                                           double *cov_out, int64_t B, void *stream) {
  using namespace aesmc;
  if (model == nullptr || mean == nullptr || cov == nullptr || mean_next == nullptr || cov_next == nullptr ||
      mean_out == nullptr || cov_out == nullptr || B < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, false)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(mean_next, 8) || !sk_aligned(cov_next, 8) ||
      !sk_aligned(mean_out, 8) || !sk_aligned(cov_out, 8))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({mean_out, cov_out}, {mean, cov, mean_next, cov_next})) return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0) return AESMC_OK;
  if (!sk_extents_supported(model->M, model->D, model->Dy) || !sk_fits_32bit(B, model->M * model->M, 1))
    return AESMC_ERR_UNSUPPORTED;
  PairSmoothArgs a;
  sk_fill_model(a, model);
  a.mean = mean, a.cov = cov, a.mean_next = mean_next, a.cov_next = cov_next, a.mean_out = mean_out, a.cov_out = cov_out;
  a.total = B * model->M * model->M;
  const int dp = sk_pad(model->D);
  const int lanes = ps_lanes(dp);
  const size_t lds = ((size_t)a.M * sk_per_regime(dp, 0) + (size_t)ps_per_lane(dp) * lanes) * sizeof(double);      // (at most 10 KB + 68 KB)
  return sk_for_extent(dp, [&](auto d) {
    return sk_launch(&switching_pair_smooth_kernel<decltype(d)::value>, dim3((unsigned)((a.total + lanes - 1) / lanes)),
                     dim3(lanes), lds, (hipStream_t)stream, a);
  });
}
