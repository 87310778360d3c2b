// The pair scores of Rao-Blackwellised backward simulation for a switching linear-Gaussian state-space model —
// aesmc_switching_backward_scores (K35) of include/aesmc_hip.h; switching_information.hip (K34) writes what it reads.
//
// Trajectory n of batch row b carries lam and the lower factor F of Om (F F^T = Om, Phi = F^T); stored particle k of step t
// carries (s, m, P, log w).  The score is the logarithm of w Pi[s, s'] times the closed-form integral of
// exp(lam^T z - 1/2 z^T Om z) against N(m, P): with h = lam - Om m, v = Phi P h and Lam = I + Phi P Phi^T,
//   log w + log Pi[s, s'] + lam^T m - 1/2 m^T Om m + 1/2 (h^T P h - v^T Lam^-1 v) - 1/2 log|Lam|.
// Lam has pivots of at least 1 (no pivot test), P is never factored (P = 0 is fine), Om is never formed.
//
//   workgroup = (batch row, a tile of 16 trajectories, 256 consecutive particles); the tile's F, lam and, for every regime s,
//               log Pi[s, s'_n] are staged into LDS once, zero-padded to the instantiation's extent DP (2, 4, 8), and read as
//               broadcasts: every lane of a wavefront reads the same address;
//   lane      = one particle: it loads its (s, m, P, log w) ONCE and walks the tile's trajectories — 16 scores for 8 + 4 +
//               8 D + 4 D (D + 1) bytes read; the scores are written [B,N,K], consecutive lanes to consecutive addresses;
//   registers   W = Phi P is formed one row at a time: row i gives row i of Lam and v_i, so m, h, Lam, one row of W and P are
//               all that is live.  At DP = 8 that is still 36 + 36 + 8 + 8 + 8 + 8 float64 = 208 registers before addresses
//               and temporaries, so the 8-wide instantiation keeps P in LDS in K31's [element][lane] layout (SkCov: 72 KB
//               per workgroup, two workgroups per compute unit).  About D^3 float64 multiply-adds per pair;
//   chains      (switching_score.hpp) every value is ONE chain of float64 __builtin_fma in the header's order; the triangular sums skip the
//               structural zeros of F, a padded term multiplies a zero by a zero.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2>      58      0        0             8
//   <4>     126      0        0             4
//   <8>     200      0        0             2       P in LDS
// (the score itself is switching_pair_score of switching_score.hpp, which K37 calls too)
// Measured (profiles/switching_smoother.txt, B = 64, K = 1024, N = 64: 4.2 million pairs): 98 us at D = 4, 342 us at D = 8.
#include "switching_host.hpp"
#include "switching_score.hpp"

namespace aesmc {

constexpr int kSbTile = 16;      // trajectories per workgroup

struct BackwardScoreArgs {
  const double *log_Pi;             // [M,M]
  const int32_t *regime_next;       // [B,N]
  const double *factor, *lambda;    // [B,N,D(D+1)/2], [B,N,D]
  const int32_t *regime;            // [B,K]
  const double *mean, *cov, *log_w; // [B,K,D], [B,K,D(D+1)/2], [B,K] or NULL
  double *scores;                   // [B,N,K]
  int32_t *flags;
  uint32_t K, N, k_tiles, n_tiles;
  int M, D;
};

// LDS: F [kSbTile][TP], lam [kSbTile][DP], log Pi[., s'_n] [kSbTile][M]; then, for DP == 8, [TP][256] covariances
template <int DP>
__global__ __launch_bounds__(kSkBlock) void switching_backward_kernel(const BackwardScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sb_smem[];
  constexpr int TP = DP * (DP + 1) / 2;
  const int M = a.M, D = a.D;
  const int TD = D * (D + 1) / 2;
  const uint32_t kt = blockIdx.x % a.k_tiles;
  const uint32_t rest = blockIdx.x / a.k_tiles;
  const uint32_t nt = rest % a.n_tiles;
  const int64_t b = rest / a.n_tiles;
  const uint32_t n0 = nt * kSbTile;
  const int count = (int)(a.N - n0 < (uint32_t)kSbTile ? a.N - n0 : (uint32_t)kSbTile);
  double *Ft = sb_smem, *lt = Ft + kSbTile * TP, *pt = lt + kSbTile * DP;
  for (int e = threadIdx.x; e < kSbTile * TP; e += kSkBlock) {
    const int nn = e / TP, el = e - nn * TP;
    Ft[e] = (nn < count && el < TD) ? a.factor[(b * a.N + n0 + nn) * TD + el] : 0.0;
  }
  for (int e = threadIdx.x; e < kSbTile * DP; e += kSkBlock) {
    const int nn = e / DP, el = e - nn * DP;
    lt[e] = (nn < count && el < D) ? a.lambda[(b * a.N + n0 + nn) * D + el] : 0.0;
  }
  for (int e = threadIdx.x; e < kSbTile * M; e += kSkBlock) {
    const int nn = e / M, s = e - nn * M;
    double v = 0.0;
    if (nn < count) {
      const int next = a.regime_next[b * a.N + n0 + nn];
      if (next < 0 || next >= M) {      // (a NaN column: every score of the trajectory is NaN)
        if (s == 0 && kt == 0) raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
        v = Num<double>::nan();
      } else {
        v = a.log_Pi[s * M + next];
      }
    }
    pt[e] = v;
  }
  __syncthreads();
  const uint32_t k = kt * kSkBlock + threadIdx.x;
  if (k >= a.K) return;
  const int64_t particle = b * a.K + k;
  double *out = a.scores + (b * a.N + n0) * a.K + k;

  int s = a.regime[particle];
  if (s < 0 || s >= M) {
    raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    for (int nn = 0; nn < count; ++nn) out[(int64_t)nn * a.K] = Num<double>::nan();
    return;
  }
  double m[DP];
  SkCov<TP, sk_cov_in_lds(DP)> P;
  P.lds = pt + kSbTile * M + threadIdx.x;
  {
    const double *mrow = a.mean + particle * D, *prow = a.cov + particle * TD;
#pragma unroll
    for (int i = 0; i < DP; ++i) m[i] = i < D ? mrow[i] : 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) P.set(e, e < TD ? prow[e] : 0.0);
  }
  const double lw = a.log_w != nullptr ? a.log_w[particle] : 0.0;
  const bool weighted = a.log_w != nullptr;

  for (int nn = 0; nn < count; ++nn) {
    out[(int64_t)nn * a.K] = switching_pair_score<DP>(Ft + nn * TP, lt + nn * DP, m, P, pt + nn * M + s, lw, weighted);
  }
}

}  // namespace aesmc

extern "C" int aesmc_switching_backward_scores(const double *log_Pi, const int32_t *regime_next, const double *factor,
                                               const double *lambda, const int32_t *regime, const double *mean,
                                               const double *cov, const double *log_w, double *scores, int32_t *flags,
                                               int64_t B, int64_t K, int64_t N, int64_t M, int64_t D, void *stream) {
  using namespace aesmc;
  if (log_Pi == nullptr || regime_next == nullptr || factor == nullptr || lambda == nullptr || regime == nullptr ||
      mean == nullptr || cov == nullptr || scores == nullptr || B < 0 || K < 0 || N < 0 || !sk_extents_positive(M, D, 1))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(log_Pi, 8) || !sk_aligned(regime_next, 4) || !sk_aligned(factor, 8) || !sk_aligned(lambda, 8) ||
      !sk_aligned(regime, 4) || !sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(log_w, 8) ||
      !sk_aligned(scores, 8) || !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({scores}, {log_Pi, regime_next, factor, lambda, regime, mean, cov, log_w}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0 || K == 0) return AESMC_OK;
  if (!sk_extents_supported(M, D, 1) || !sk_fits_32bit(B, K, kSkTriMax) || !sk_fits_32bit(B, N, kSkTriMax) ||
      !sk_fits_32bit(B, N, K))      // (the last: B N K scores)
    return AESMC_ERR_UNSUPPORTED;
  BackwardScoreArgs a;
  a.log_Pi = log_Pi, a.regime_next = regime_next, a.factor = factor, a.lambda = lambda;
  a.regime = regime, a.mean = mean, a.cov = cov, a.log_w = log_w;
  a.scores = scores, a.flags = flags;
  a.K = (uint32_t)K, a.N = (uint32_t)N;
  a.k_tiles = (uint32_t)((K + kSkBlock - 1) / kSkBlock), a.n_tiles = (uint32_t)((N + kSbTile - 1) / kSbTile);
  a.M = (int)M, a.D = (int)D;
  const int dp = sk_pad(D);
  const int tp = dp * (dp + 1) / 2;
  const size_t lds = ((size_t)kSbTile * (tp + dp + a.M) + (sk_cov_in_lds(dp) ? (size_t)tp * kSkBlock : 0)) * sizeof(double);
  const dim3 grid((unsigned)(B * a.n_tiles * a.k_tiles));      // (at most B N K workgroups: within 32 bits by the check above)
  return sk_for_extent(dp, [&](auto d) {
    return sk_launch(&switching_backward_kernel<decltype(d)::value>, grid, dim3(kSkBlock), lds, (hipStream_t)stream, a);
  });
}
