// What the kernels of the switching linear-Gaussian filters share (switching_kalman.hip: K31, K33 and their masked form K39;
// switching_lookahead.hip: K32 and K40): the limits, the packed-triangle index, where a lane keeps its predicted covariance, and the model's staging into LDS.
// What their C entries share on the host (checks, dispatch, launch) is switching_host.hpp.
#pragma once
#include "common.hpp"

namespace aesmc {

constexpr int kSkBlock = 256;
constexpr int kSkMaxDim = 8;        // D and Dy
constexpr int kSkMaxRegimes = 16;
constexpr double kHalfLog2Pi = 0.9189385332046727;

// whether an instantiation keeps the predicted covariance in LDS (see SkCov)
__host__ __device__ constexpr bool sk_cov_in_lds(int dp) { return dp == 8; }
// The compiler otherwise keeps every model value it has read once in a register for its later uses (128 VGPRs per 8 x 8
// matrix): after this it reads LDS again
#define SK_REREAD_LDS() asm volatile("" ::: "memory")

__host__ __device__ constexpr int sk_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// A lane's packed predicted covariance P-: in registers, or (the 8-wide instantiations, which would spill) in LDS in an
// [element][lane] layout — consecutive lanes on consecutive banks, no conflicts; Lanes: the workgroup's size (K37 has two)
template <int TP, bool InLds, int Lanes = kSkBlock> struct SkCov {
  double reg[InLds ? 1 : TP];
  double *lds;
  __device__ __forceinline__ double get(int e) const {
    if constexpr (InLds) return lds[e * Lanes];
    else return reg[e];
  }
  __device__ __forceinline__ void set(int e, double v) {
    if constexpr (InLds) lds[e * Lanes] = v;
    else reg[e] = v;
  }
};

// values per regime of the staged model: A [DP,DP], b [DP], q^2 [DP], C [DYP,DP], d [DYP], r^2 [DYP]
__host__ __device__ constexpr int sk_per_regime(int dp, int dyp) { return dp * dp + 2 * dp + dyp * dp + 2 * dyp; }

// Stages every regime's block into `mdl` as float64, zero-padded to the instantiation's extents (r^2 padded with ONE: the
// padded pivots are 1, their logarithms 0).  The whole workgroup calls it; the caller places the barrier.  Lanes: the
// workgroup's size (K48 has two)
template <int DP, int DYP, int Lanes = kSkBlock>
__device__ __forceinline__ void sk_stage_model(double *mdl, int M, int D, int Dy, const double *A, const double *b,
                                               const double *q, const double *C, const double *d, const double *r) {
  constexpr int kPer = sk_per_regime(DP, DYP);
  for (int e = threadIdx.x; e < M * kPer; e += Lanes) {
    const int s = e / kPer;
    int o = e - s * kPer;
    double v;
    if (o < DP * DP) {
      const int i = o / DP, l = o - i * DP;
      v = (i < D && l < D) ? A[(s * D + i) * D + l] : 0.0;
    } else if ((o -= DP * DP) < DP) {
      v = o < D ? b[s * D + o] : 0.0;
    } else if ((o -= DP) < DP) {
      const double qv = o < D ? q[s * D + o] : 0.0;
      v = qv * qv;
    } else if ((o -= DP) < DYP * DP) {
      const int i = o / DP, l = o - i * DP;
      v = (i < Dy && l < D) ? C[(s * Dy + i) * D + l] : 0.0;
    } else if ((o -= DYP * DP) < DYP) {
      v = o < Dy ? d[s * Dy + o] : 0.0;
    } else {
      o -= DYP;
      const double rv = o < Dy ? r[s * Dy + o] : 1.0;
      v = rv * rv;
    }
    mdl[e] = v;
  }
}

}  // namespace aesmc
