// The adjoint of one step of K31 with the regime given — aesmc_switching_kalman_step_backward (K52) and, under K39's mask,
// aesmc_switching_kalman_masked_step_backward (K53) of include/aesmc_hip.h — for the gradient of the collapsed-mixture
// evidence (aesmc_amd.rao_blackwell.collapsed_switching_log_likelihood).  switching_kalman.hip is not touched; what the two
// share is switching_kalman.hpp (the staged model, SkCov, sk_tri) and switching_host.hpp (checks, dispatch, launch).
//
// One lane per slot of the flattened [B K] range.  The lane RECOMPUTES the forward chains of its slot in K31's order (predict,
// innovation, U = C P-, S, the factor Lam, v = Lam^-1 e, V = Lam^-1 U) — nothing comes from a tape — and then, with g, mu, G the
// gradients arriving at the log-weight, the mean and the covariance (G dense and symmetric: a packed off-diagonal element
// stands for both positions, so it enters halved and leaves doubled):
//   z = V mu;   alpha = Lam^-T v;   t = Lam^-T z;   ebar = t - g alpha
//   Y = v mu^T - 2 V G;                         Ubar = Lam^-T Y
//   Shat = g/2 (v v^T - I) - sym(z v^T) + (V G) V^T;      Sbar = Lam^-T Shat Lam^-1      (two triangular solves: no S^-1)
//   Hhat = Ubar + Sbar C;      Pbar- = G + sym(C^T Hhat);      mbar- = mu - C^T ebar
//   Cbar = (Hhat + Sbar C) P- - ebar m-^T;      dbar = -ebar;      rbar = 2 r o diag Sbar
//   later steps:  Abar = 2 Pbar- (A P) + mbar- m^T;  bbar = mbar-;  qbar = 2 q o diag Pbar-;  mbar = A^T mbar-;  Pbar = A^T Pbar- A
//   step 0:       m0bar = mbar-;  s0bar = 2 s0 o diag Pbar-
// Masked: a deleted component has e, its row of U and its row and column of S selected as K39 selects them; its diagonal
// entry of Shat is selected to 0, and with it every gradient of its row of C, d and r is exactly 0.
//
//   workgroup = 256 lanes with every matrix in registers where both padded extents are at most 4; where one of them is 8,
//               64 lanes with P-, G (which becomes Pbar-), the factor, V (whose place Sbar takes) and Y (which becomes Ubar
//               and Hhat) in LDS in SkCov's [element][lane] layout — 236 values per lane at <8,8>: 118 KB beside the model's
//               20 KB at most.  A collapsed pass launches B M^2 slots: occupancy is not the concern.
//   model     staged by sk_stage_model and read as broadcasts; q, r and s0 themselves (the staged ones are squared) from memory.
//   sums      the per-regime gradients are not added here: every slot leaves ITS row (A, b, q, C, d, r, m0, s0: D^2 + 2 D +
//             Dy D + 2 Dy + 2 D values) in the workspace, and two finishing launches add them per regime and element: the slots
//             are cut into min(64, ceil(B K / 256)) consecutive parts, a workgroup per part adds sixteen consecutive runs
//             of its slots in ascending order and then the sixteen sums in ascending order, and the second launch adds the
//             parts in ascending order.  No floating-point atomics: the same inputs and extents give the same bits.
// A slot whose three arriving gradients are all exactly zero writes exact zeros and computes nothing (its forward may be
// NaN: K31's outputs under an impossible regime).  A regime outside [0, M) raises AESMC_FLAG_INDEX_OUT_OF_RANGE, writes NaN
// to the slot's rows of grad_mean_in and grad_cov_in and adds nothing to any regime.  A pivot that is not positive gives NaN.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950; K52 / K53 where they differ):
//   <DP,DYP>  lanes   VGPRs      AGPRs     scratch B/lane  waves/SIMD
//   <2,2>      256      88          0           0             5
//   <2,4>      256     144          0           0             3
//   <2,8>       64     252          0           0             2       matrices in LDS
//   <4,2>      256   146 / 148      0           0             3
//   <4,4>      256     224          0           0             2
//   <4,8>       64     256       78 / 80        0             1       matrices in LDS
//   <8,2>       64     256         130          0             1       matrices in LDS
//   <8,4>       64     256         128          0             1       matrices in LDS
//   <8,8>       64     256      204 / 208       0             1       matrices in LDS
//   partial   1024      36          0           0             8       8 KB of static LDS; the second finishing launch: 64 lanes
// No instantiation uses scratch.  The 64-lane instantiations are one wavefront per workgroup, so the unified register file
// gives a lane up to 512 registers: the compiler keeps what it has read from LDS in accumulation registers instead of
// reading it again (moves, not spills).
#include "switching_host.hpp"

namespace aesmc {

struct SkBackwardArgs {
  const double *m0, *s0;
  const double *A, *b, *q, *C, *d, *r;
  const int32_t *regime;               // [B,K]: the regime each slot used
  const double *mean_in, *cov_in;      // NULL: step 0
  const void *y;
  const uint8_t *observed;             // K53: [B,Dy]
  const double *grad_mean, *grad_cov, *grad_lw;
  double *grad_mean_in, *grad_cov_in;  // may be NULL
  double *rows;                        // [B K][row] or NULL
  int32_t *flags;
  int64_t N;
  uint32_t K;
  int M, D, Dy, y_is_float;
};

__host__ __device__ constexpr bool skb_in_lds(int dp, int dyp) { return dp == 8 || dyp == 8; }
__host__ __device__ constexpr int skb_lanes(int dp, int dyp) { return skb_in_lds(dp, dyp) ? 64 : kSkBlock; }
__host__ __device__ constexpr int skb_wide(int dp, int dyp) { return dyp * (dp > dyp ? dp : dyp); }
// LDS values per lane: P-, G, the factor, V / Sbar, Y / Hhat
__host__ __device__ constexpr int skb_per_lane(int dp, int dyp) {
  return skb_in_lds(dp, dyp) ? dp * (dp + 1) + dyp * (dyp + 1) / 2 + skb_wide(dp, dyp) + dyp * dp : 0;
}
__host__ __device__ constexpr int64_t skb_row(int64_t D, int64_t Dy) { return D * D + 2 * D + Dy * D + 2 * Dy + 2 * D; }

template <int DP, int DYP, bool Masked>
__global__ __launch_bounds__(skb_lanes(DP, DYP)) void switching_kalman_backward_kernel(const SkBackwardArgs a) {
  extern __shared__ __attribute__((aligned(16))) double skb_smem[];
  constexpr int kLanes = skb_lanes(DP, DYP);
  constexpr bool kLds = skb_in_lds(DP, DYP);
  constexpr int kPer = sk_per_regime(DP, DYP);
  constexpr int TP = DP * (DP + 1) / 2, TY = DYP * (DYP + 1) / 2;
  constexpr int XW = DP > DYP ? DP : DYP;      // the row length of V's place (V: DP of it; Sbar: DYP)
  const int M = a.M, D = a.D, Dy = a.Dy;
  const bool later = a.mean_in != nullptr;
  sk_stage_model<DP, DYP, kLanes>(skb_smem, M, D, Dy, a.A, a.b, a.q, a.C, a.d, a.r);
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (n >= a.N) return;      // (no barrier follows; a lane's slots in LDS are its own)
  const int64_t b = n / a.K;
  const int TD = D * (D + 1) / 2;
  const int row = (int)skb_row(D, Dy);
  double *min_out = a.grad_mean_in != nullptr ? a.grad_mean_in + n * D : nullptr;
  double *pin_out = a.grad_cov_in != nullptr ? a.grad_cov_in + n * TD : nullptr;
  double *out = a.rows != nullptr ? a.rows + n * row : nullptr;
  const auto fill = [&](double slot_value, double row_value) {
    if (min_out != nullptr)
      for (int i = 0; i < D; ++i) min_out[i] = slot_value;
    if (pin_out != nullptr)
      for (int e = 0; e < TD; ++e) pin_out[e] = slot_value;
    if (out != nullptr)
      for (int e = 0; e < row; ++e) out[e] = row_value;
  };
  const int s = a.regime[n];
  if (s < 0 || s >= M) {
    raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    fill(Num<double>::nan(), 0.0);
    return;
  }

  // ---- the arriving gradients; G in its dense symmetric form ------------------------------------------------------------------
  double gm[DP];
  SkCov<TP, kLds, kLanes> Pm, G;
  SkCov<TY, kLds, kLanes> L;
  SkCov<DYP * XW, kLds, kLanes> X;       // V [DYP][DP] by rows of XW, later Sbar [DYP][DYP]
  SkCov<DYP * DP, kLds, kLanes> H;       // Y, then Ubar, then Hhat
  Pm.lds = skb_smem + M * kPer + threadIdx.x;
  G.lds = Pm.lds + TP * kLanes;
  L.lds = G.lds + TP * kLanes;
  X.lds = L.lds + TY * kLanes;
  H.lds = X.lds + DYP * XW * kLanes;
  const double gl = a.grad_lw[n];
  bool any = gl != 0.0;
  {
    const double *grow = a.grad_mean + n * D, *crow = a.grad_cov + n * TD;
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      gm[i] = i < D ? grow[i] : 0.0;
      any = any || gm[i] != 0.0;
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const double c = sk_tri(i, j) < TD ? crow[sk_tri(i, j)] : 0.0;
        any = any || c != 0.0;
        G.set(sk_tri(i, j), i == j ? c : 0.5 * c);
      }
    }
  }
  if (!any) {
    fill(0.0, 0.0);
    return;
  }

  const double *Am = skb_smem + s * kPer, *bv = Am + DP * DP, *q2 = bv + DP, *Cm = q2 + DP, *dv = Cm + DYP * DP, *r2 = dv + DYP;

  // ---- the forward chains, as K31 forms them: predict ----------------------------------------------------------------------------
  double mp[DP];
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
    double W[DP][DP];
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

  // ---- innovation, U = C P- (into V's place), S (into the factor's place) -----------------------------------------------------------
  SK_REREAD_LDS();
  double v[DYP], yv[DYP];
  bool ob[DYP];
  if constexpr (Masked) {
    const uint8_t *orow = a.observed + b * Dy;
#pragma unroll
    for (int i = 0; i < DYP; ++i) ob[i] = i < Dy ? orow[i] != 0 : false;
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
    v[i] = Masked && !ob[i] ? 0.0 : acc;
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double w = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) w = __builtin_fma(Cm[i * DP + c], Pm.get(sk_tri(c, l)), w);
      X.set(i * XW + l, Masked && !ob[i] ? 0.0 : w);
    }
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double w = i == j ? r2[i] : 0.0;
#pragma unroll
      for (int l = 0; l < DP; ++l) w = __builtin_fma(Cm[i * DP + l], X.get(j * XW + l), w);
      L.set(sk_tri(i, j), Masked && !(ob[i] && ob[j]) ? (i == j ? 1.0 : 0.0) : w);
    }
  }

  // ---- Lam = chol(S) in place; inv[j] = 1 / Lam_jj ---------------------------------------------------------------------------------
  double inv[DYP];
  bool positive = true;
#pragma unroll
  for (int j = 0; j < DYP; ++j) {
    double pivot = L.get(sk_tri(j, j));
#pragma unroll
    for (int c = 0; c < j; ++c) pivot = __builtin_fma(-L.get(sk_tri(j, c)), L.get(sk_tri(j, c)), pivot);
    positive = positive && pivot > 0.0;
    const double ljj = __builtin_sqrt(pivot);
    L.set(sk_tri(j, j), ljj);
    inv[j] = 1.0 / ljj;
#pragma unroll
    for (int i = j + 1; i < DYP; ++i) {
      double acc = L.get(sk_tri(i, j));
#pragma unroll
      for (int c = 0; c < j; ++c) acc = __builtin_fma(-L.get(sk_tri(i, c)), L.get(sk_tri(j, c)), acc);
      L.set(sk_tri(i, j), acc * inv[j]);
    }
  }
  if (!positive) {
    fill(Num<double>::nan(), Num<double>::nan());
    return;
  }

  // ---- v = Lam^-1 e, V = Lam^-1 U (in place) ------------------------------------------------------------------------------------------
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    double acc = v[i];
#pragma unroll
    for (int c = 0; c < i; ++c) acc = __builtin_fma(-L.get(sk_tri(i, c)), v[c], acc);
    v[i] = acc * inv[i];
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double w = X.get(i * XW + l);
#pragma unroll
      for (int c = 0; c < i; ++c) w = __builtin_fma(-L.get(sk_tri(i, c)), X.get(c * XW + l), w);
      X.set(i * XW + l, w * inv[i]);
    }
  }

  // ---- z = V mu;  Y = v mu^T - 2 V G;  Shat = g/2 (v v^T - I) - sym(z v^T) + (V G) V^T ---------------------------------------------
  double z[DYP], Sh[TY];
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < DP; ++l) acc = __builtin_fma(X.get(i * XW + l), gm[l], acc);
    z[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    double vg[DP];
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) acc = __builtin_fma(X.get(i * XW + c), G.get(sk_tri(c, l)), acc);
      vg[l] = acc;
      H.set(i * DP + l, __builtin_fma(v[i], gm[l], -2.0 * acc));
    }
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double acc = 0.5 * gl * (v[i] * v[j] - (i == j ? 1.0 : 0.0)) - 0.5 * (z[i] * v[j] + z[j] * v[i]);
#pragma unroll
      for (int l = 0; l < DP; ++l) acc = __builtin_fma(vg[l], X.get(j * XW + l), acc);
      Sh[sk_tri(i, j)] = (Masked && i == j && !ob[i]) ? 0.0 : acc;
    }
  }

  // ---- alpha = Lam^-T v, t = Lam^-T z: ebar = t - g alpha (into z);  Ubar = Lam^-T Y (in place, from the last row up) ----------------
#pragma unroll
  for (int i = DYP - 1; i >= 0; --i) {
    double acc = v[i], w = z[i];
#pragma unroll
    for (int c = i + 1; c < DYP; ++c) {
      acc = __builtin_fma(-L.get(sk_tri(c, i)), v[c], acc);
      w = __builtin_fma(-L.get(sk_tri(c, i)), z[c], w);
    }
    v[i] = acc * inv[i];      // alpha
    z[i] = w * inv[i];        // t
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double u = H.get(i * DP + l);
#pragma unroll
      for (int c = i + 1; c < DYP; ++c) u = __builtin_fma(-L.get(sk_tri(c, i)), H.get(c * DP + l), u);
      H.set(i * DP + l, u * inv[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < DYP; ++i) z[i] = __builtin_fma(-gl, v[i], z[i]);      // ebar

  // ---- Sbar = Lam^-T Shat Lam^-1 in V's place: rows from the last up, then columns from the last down -----------------------------
#pragma unroll
  for (int i = DYP - 1; i >= 0; --i) {
#pragma unroll
    for (int j = 0; j < DYP; ++j) {
      double acc = Sh[sk_tri(i, j)];
#pragma unroll
      for (int c = i + 1; c < DYP; ++c) acc = __builtin_fma(-L.get(sk_tri(c, i)), X.get(c * XW + j), acc);
      X.set(i * XW + j, acc * inv[i]);
    }
  }
#pragma unroll
  for (int j = DYP - 1; j >= 0; --j) {
#pragma unroll
    for (int i = 0; i < DYP; ++i) {
      double acc = X.get(i * XW + j);
#pragma unroll
      for (int c = j + 1; c < DYP; ++c) acc = __builtin_fma(-X.get(i * XW + c), L.get(sk_tri(c, j)), acc);
      X.set(i * XW + j, acc * inv[j]);
    }
  }

  // ---- Hhat = Ubar + Sbar C;  Cbar = (Hhat + Sbar C) P- - ebar m-^T;  dbar = -ebar;  rbar = 2 r o diag Sbar -------------------------
  SK_REREAD_LDS();
  // where the row's parts begin (offsets, not pointers: `out` is NULL when no sum is wanted)
  const int fA = 0, fb = D * D, fq = fb + D, fC = fq + D, fd = fC + Dy * D, fr = fd + Dy, fm0 = fr + Dy, fs0 = fm0 + D;
#pragma unroll
  for (int i = 0; i < DYP; ++i) {
    double qrow[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) {
      double sc = 0.0;
#pragma unroll
      for (int j = 0; j < DYP; ++j) sc = __builtin_fma(X.get(i * XW + j), Cm[j * DP + c], sc);
      const double h = H.get(i * DP + c) + sc;
      H.set(i * DP + c, h);
      qrow[c] = h + sc;
    }
    if (out != nullptr && i < Dy) {
      const bool dead = Masked && !ob[i];
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        double acc = -z[i] * mp[l];
#pragma unroll
        for (int c = 0; c < DP; ++c) acc = __builtin_fma(qrow[c], Pm.get(sk_tri(c, l)), acc);
        if (l < D) out[fC + i * D + l] = dead ? 0.0 : acc;
      }
      out[fd + i] = dead ? 0.0 : -z[i];
      out[fr + i] = dead ? 0.0 : 2.0 * a.r[s * Dy + i] * X.get(i * XW + i);
    }
  }

  // ---- mbar- = mu - C^T ebar;  Pbar- = G + sym(C^T Hhat) (in G's place) ------------------------------------------------------------
  double mb[DP];
#pragma unroll
  for (int l = 0; l < DP; ++l) {
    double acc = gm[l];
#pragma unroll
    for (int i = 0; i < DYP; ++i) acc = __builtin_fma(-Cm[i * DP + l], z[i], acc);
    mb[l] = acc;
#pragma unroll
    for (int j = 0; j <= l; ++j) {
      double w = 0.0;
#pragma unroll
      for (int i = 0; i < DYP; ++i) {
        w = __builtin_fma(Cm[i * DP + l], H.get(i * DP + j), w);
        w = __builtin_fma(Cm[i * DP + j], H.get(i * DP + l), w);
      }
      G.set(sk_tri(l, j), __builtin_fma(0.5, w, G.get(sk_tri(l, j))));
    }
  }

  if (!later) {
    if (out != nullptr) {
      for (int e = 0; e < D * D + 2 * D; ++e) out[fA + e] = 0.0;
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < D) out[fm0 + i] = mb[i], out[fs0 + i] = 2.0 * a.s0[i] * G.get(sk_tri(i, i));
    }
    return;
  }

  // ---- through the predict: P's place takes the slot's P again, W = A P --------------------------------------------------------------
  SK_REREAD_LDS();
  {
    const double *prow = a.cov_in + n * TD;
#pragma unroll
    for (int e = 0; e < TP; ++e) Pm.set(e, e < TD ? prow[e] : 0.0);
  }
  if (out != nullptr) {
    const double *mrow = a.mean_in + n * D;
    double mi[DP], W[DP][DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) mi[i] = i < D ? mrow[i] : 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i) {
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) acc = __builtin_fma(Am[i * DP + c], Pm.get(sk_tri(c, l)), acc);
        W[i][l] = acc;
      }
    }
#pragma unroll
    for (int i = 0; i < DP; ++i) {
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) acc = __builtin_fma(G.get(sk_tri(i, c)), W[c][l], acc);
        if (i < D && l < D) out[fA + i * D + l] = __builtin_fma(mb[i], mi[l], 2.0 * acc);
      }
      if (i < D) out[fb + i] = mb[i], out[fq + i] = 2.0 * a.q[s * D + i] * G.get(sk_tri(i, i)), out[fm0 + i] = 0.0, out[fs0 + i] = 0.0;
    }
  }
  if (min_out != nullptr) {
#pragma unroll
    for (int l = 0; l < DP; ++l) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < DP; ++i) acc = __builtin_fma(Am[i * DP + l], mb[i], acc);
      if (l < D) min_out[l] = acc;
    }
  }
  if (pin_out != nullptr) {
    SK_REREAD_LDS();
    double T2[DP][DP];      // Pbar- A
#pragma unroll
    for (int i = 0; i < DP; ++i) {
#pragma unroll
      for (int l = 0; l < DP; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) acc = __builtin_fma(G.get(sk_tri(i, c)), Am[c * DP + l], acc);
        T2[i][l] = acc;
      }
    }
#pragma unroll
    for (int l = 0; l < DP; ++l) {
#pragma unroll
      for (int j = 0; j <= l; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < DP; ++i) acc = __builtin_fma(Am[i * DP + l], T2[i][j], acc);
        if (sk_tri(l, j) < TD) pin_out[sk_tri(l, j)] = l == j ? acc : 2.0 * acc;
      }
    }
  }
}

// ---- the finishing launches: the slots are cut into `parts` consecutive parts (a grid axis); a workgroup adds, per regime and
// element, the slots of sixteen consecutive runs of its part in ascending order and then the sixteen sums in ascending order,
// and leaves the part's sum behind the rows in the workspace; the second launch adds the parts in ascending order.  One fixed
// order for given extents
constexpr int kSkbRuns = 16, kSkbElements = 64, kSkbMaxParts = 64, kSkbPartSlots = 256;

struct SkFinishArgs {
  const double *rows;
  double *partial;      // [parts][M][row]
  const int32_t *regime;
  double *grad_A, *grad_b, *grad_q, *grad_C, *grad_d, *grad_r, *grad_m0, *grad_s0;
  int64_t N;
  int M, D, Dy, parts;
};

static inline int skb_parts(int64_t N) {
  const int64_t parts = (N + kSkbPartSlots - 1) / kSkbPartSlots;
  return (int)(parts < 1 ? 1 : parts > kSkbMaxParts ? kSkbMaxParts : parts);
}

__global__ __launch_bounds__(kSkbRuns *kSkbElements) void switching_kalman_backward_partial_kernel(const SkFinishArgs a) {
  __shared__ double part[kSkbRuns][kSkbElements];
  const int lane = threadIdx.x % kSkbElements, run = threadIdx.x / kSkbElements;
  const int el = blockIdx.x * kSkbElements + lane, s = blockIdx.y, p = blockIdx.z;
  const int row = (int)skb_row(a.D, a.Dy), per = row - 2 * a.D;
  const bool whole = el >= per;      // m0 and s0: every slot, by the workgroups of regime 0
  double acc = 0.0;
  if (el < row && (!whole || s == 0)) {
    const int64_t span = (a.N + a.parts - 1) / a.parts;
    const int64_t first = p * span, last = first + span < a.N ? first + span : a.N;
    const int64_t chunk = (span + kSkbRuns - 1) / kSkbRuns;
    const int64_t lo = first + run * chunk, hi = lo + chunk < last ? lo + chunk : last;
    for (int64_t n = lo; n < hi; ++n)
      if (whole || a.regime[n] == s) acc = acc + a.rows[n * row + el];
  }
  part[run][lane] = acc;
  __syncthreads();
  if (run != 0 || el >= row) return;
  double total = part[0][lane];
  for (int k = 1; k < kSkbRuns; ++k) total = total + part[k][lane];
  a.partial[((int64_t)p * a.M + s) * row + el] = total;
}

__global__ __launch_bounds__(kSkbElements) void switching_kalman_backward_finish_kernel(const SkFinishArgs a) {
  const int el = blockIdx.x * kSkbElements + threadIdx.x, s = blockIdx.y;
  const int D = a.D, Dy = a.Dy;
  const int row = (int)skb_row(D, Dy), per = row - 2 * D;
  const bool whole = el >= per;
  if (el >= row || (whole && s != 0)) return;
  double total = 0.0;
  for (int p = 0; p < a.parts; ++p) total = total + a.partial[((int64_t)p * a.M + s) * row + el];
  int o = el;
  double *dst;
  if (o < D * D) dst = a.grad_A ? a.grad_A + s * D * D : nullptr;
  else if ((o -= D * D) < D) dst = a.grad_b ? a.grad_b + s * D : nullptr;
  else if ((o -= D) < D) dst = a.grad_q ? a.grad_q + s * D : nullptr;
  else if ((o -= D) < Dy * D) dst = a.grad_C ? a.grad_C + s * Dy * D : nullptr;
  else if ((o -= Dy * D) < Dy) dst = a.grad_d ? a.grad_d + s * Dy : nullptr;
  else if ((o -= Dy) < Dy) dst = a.grad_r ? a.grad_r + s * Dy : nullptr;
  else if ((o -= Dy) < D) dst = a.grad_m0;
  else o -= D, dst = a.grad_s0;
  if (dst != nullptr) dst[o] = total;
}

static int skb_step(bool masked, const uint8_t *observed, int y_dtype, const aesmc_switching_model *model,
                    const int32_t *regime, const double *mean_in, const double *cov_in, const void *y,
                    const double *grad_mean, const double *grad_cov, const double *grad_log_weight, double *grad_mean_in,
                    double *grad_cov_in, double *grad_m0, double *grad_s0, double *grad_A, double *grad_b, double *grad_q,
                    double *grad_C, double *grad_d, double *grad_r, void *workspace, int64_t workspace_bytes, int32_t *flags,
                    int64_t B, int64_t K, void *stream) {
  if (model == nullptr || regime == nullptr || grad_mean == nullptr || grad_cov == nullptr || grad_log_weight == nullptr ||
      B < 0 || K < 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  const bool later = mean_in != nullptr;
  if (later != (cov_in != nullptr)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_observation(y, y_dtype) || !sk_extents_positive(model->M, model->D, model->Dy) || !sk_model_operands(model, true))
    return AESMC_ERR_INVALID_ARGUMENT;
  double *const reduced[] = {grad_m0, grad_s0, grad_A, grad_b, grad_q, grad_C, grad_d, grad_r};
  bool reduces = false;
  for (double *p : reduced) reduces = reduces || p != nullptr;
  if (!reduces && grad_mean_in == nullptr && grad_cov_in == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  // step 0 has no stored state to give a gradient to; a later step does not read the initial state
  if (later ? (grad_m0 != nullptr || grad_s0 != nullptr) : (grad_mean_in != nullptr || grad_cov_in != nullptr))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (masked && observed == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(regime, 4) || !sk_aligned(mean_in, 8) || !sk_aligned(cov_in, 8) || !sk_aligned(grad_mean, 8) ||
      !sk_aligned(grad_cov, 8) || !sk_aligned(grad_log_weight, 8) || !sk_aligned(grad_mean_in, 8) ||
      !sk_aligned(grad_cov_in, 8) || !sk_aligned(workspace, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  for (double *p : reduced)
    if (!sk_aligned(p, 8)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({grad_mean_in, grad_cov_in, grad_m0, grad_s0, grad_A, grad_b, grad_q, grad_C, grad_d, grad_r,
                            reduces ? workspace : nullptr},
                           {regime, mean_in, cov_in, y, observed, grad_mean, grad_cov, grad_log_weight, model->m0, model->s0,
                            model->A, model->b, model->q, model->C, model->d, model->r}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (reduces && workspace == nullptr) return AESMC_ERR_WORKSPACE;
  if (B == 0 || K == 0) return AESMC_OK;      // (the reduced gradients of an empty launch are not written)
  if (!sk_extents_supported(model->M, model->D, model->Dy) || !sk_fits_32bit(B, K, skb_row(kSkMaxDim, kSkMaxDim)))
    return AESMC_ERR_UNSUPPORTED;
  if (reduces && workspace_bytes < aesmc_switching_backward_workspace_bytes(B, K, model->D, model->Dy)) return AESMC_ERR_WORKSPACE;
  SkBackwardArgs a;
  sk_fill_model(a, model);
  a.m0 = model->m0, a.s0 = model->s0;
  a.regime = regime, a.mean_in = mean_in, a.cov_in = cov_in, a.y = y;
  a.observed = masked ? observed : nullptr;
  a.grad_mean = grad_mean, a.grad_cov = grad_cov, a.grad_lw = grad_log_weight;
  a.grad_mean_in = grad_mean_in, a.grad_cov_in = grad_cov_in;
  a.rows = reduces ? (double *)workspace : nullptr;
  a.flags = flags;
  a.N = B * K, a.K = (uint32_t)K;
  a.y_is_float = y_dtype == AESMC_F32;
  const int dp = sk_pad(model->D), dyp = sk_pad(model->Dy);
  const int lanes = skb_lanes(dp, dyp);
  const size_t lds = ((size_t)a.M * sk_per_regime(dp, dyp) + (size_t)skb_per_lane(dp, dyp) * lanes) * sizeof(double);
  const int status = sk_for_extents(dp, dyp, [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      return sk_launch(&switching_kalman_backward_kernel<decltype(d)::value, decltype(dy)::value, decltype(m)::value>,
                       dim3((unsigned)((a.N + lanes - 1) / lanes)), dim3(lanes), lds, (hipStream_t)stream, a);
    });
  });
  if (status != AESMC_OK || !reduces) return status;
  SkFinishArgs f;
  f.rows = a.rows, f.partial = a.rows + a.N * skb_row(a.D, a.Dy), f.regime = regime;
  f.grad_A = grad_A, f.grad_b = grad_b, f.grad_q = grad_q, f.grad_C = grad_C, f.grad_d = grad_d, f.grad_r = grad_r;
  f.grad_m0 = grad_m0, f.grad_s0 = grad_s0;
  f.N = a.N, f.M = a.M, f.D = a.D, f.Dy = a.Dy, f.parts = skb_parts(a.N);
  const unsigned tiles = (unsigned)((skb_row(a.D, a.Dy) + kSkbElements - 1) / kSkbElements);
  const int partial = sk_launch(&switching_kalman_backward_partial_kernel, dim3(tiles, (unsigned)a.M, (unsigned)f.parts),
                                dim3(kSkbRuns * kSkbElements), 0, (hipStream_t)stream, f);
  if (partial != AESMC_OK) return partial;
  return sk_launch(&switching_kalman_backward_finish_kernel, dim3(tiles, (unsigned)a.M), dim3(kSkbElements), 0,
                   (hipStream_t)stream, f);
}

}  // namespace aesmc

extern "C" int64_t aesmc_switching_backward_workspace_bytes(int64_t B, int64_t K, int64_t D, int64_t Dy) {
  if (B < 0 || K < 0 || D < 1 || Dy < 1 || D > aesmc::kSkMaxDim || Dy > aesmc::kSkMaxDim || B > 0x7fffffffLL || K > 0x7fffffffLL)
    return 0;
  if (B == 0 || K == 0) return 0;
  // the slots' rows, then the parts' sums for the largest M
  return (B * K + (int64_t)aesmc::kSkbMaxParts * aesmc::kSkMaxRegimes) * aesmc::skb_row(D, Dy) * (int64_t)sizeof(double);
}

extern "C" int aesmc_switching_kalman_step_backward(int y_dtype, const aesmc_switching_model *model, const int32_t *regime,
                                                    const double *mean_in, const double *cov_in, const void *y,
                                                    const double *grad_mean, const double *grad_cov,
                                                    const double *grad_log_weight, double *grad_mean_in, double *grad_cov_in,
                                                    double *grad_m0, double *grad_s0, double *grad_A, double *grad_b,
                                                    double *grad_q, double *grad_C, double *grad_d, double *grad_r,
                                                    void *workspace, int64_t workspace_bytes, int32_t *flags, int64_t B,
                                                    int64_t K, void *stream) {
  return aesmc::skb_step(false, nullptr, y_dtype, model, regime, mean_in, cov_in, y, grad_mean, grad_cov, grad_log_weight,
                         grad_mean_in, grad_cov_in, grad_m0, grad_s0, grad_A, grad_b, grad_q, grad_C, grad_d, grad_r, workspace,
                         workspace_bytes, flags, B, K, stream);
}

extern "C" int aesmc_switching_kalman_masked_step_backward(int y_dtype, const aesmc_switching_model *model,
                                                           const int32_t *regime, const double *mean_in, const double *cov_in,
                                                           const void *y, const uint8_t *observed, const double *grad_mean,
                                                           const double *grad_cov, const double *grad_log_weight,
                                                           double *grad_mean_in, double *grad_cov_in, double *grad_m0,
                                                           double *grad_s0, double *grad_A, double *grad_b, double *grad_q,
                                                           double *grad_C, double *grad_d, double *grad_r, void *workspace,
                                                           int64_t workspace_bytes, int32_t *flags, int64_t B, int64_t K,
                                                           void *stream) {
  return aesmc::skb_step(true, observed, y_dtype, model, regime, mean_in, cov_in, y, grad_mean, grad_cov, grad_log_weight,
                         grad_mean_in, grad_cov_in, grad_m0, grad_s0, grad_A, grad_b, grad_q, grad_C, grad_d, grad_r, workspace,
                         workspace_bytes, flags, B, K, stream);
}
