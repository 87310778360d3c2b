// The adjoint of the moment-matching collapse K50 — aesmc_switching_collapse_backward (K54) of include/aesmc_hip.h — for the
// gradient of the collapsed-mixture evidence.  switching_collapse.hip is not touched.
//
// Group (b,g): N components (lw_n, m_n, P_n), w_n their normalised weights, mean and d_n = m_n - mean as K50 forms them (the
// same chains, recomputed); abar, mu and c the gradients arriving at log_mass, mean_out and cov_out (c packed: an
// off-diagonal element stands for both positions, so <c, P> below is the sum over the PACKED elements):
//   grad_cov_n  = w_n c
//   grad_mean_n = w_n (mu + 2 sym(c) d_n)
//   omega_n     = <mu, d_n> + <c, P_n + d_n d_n^T>      (centred: sum_n w_n <mu, d_n> = 0, so this is the header's omega_n less a
//                                                        constant, which the next line removes whichever way it is written)
//   grad_lw_n   = w_n (abar + omega_n - sum_k w_k omega_k)
// Dense form: one lane per group.  Shared form (stride 0: the row's N components under every one of its G weight rows): one
// lane per BATCH ROW, which walks its groups in ascending order and adds each group's component gradients to the row's in
// memory (group 0 stores, the others load, add and store) — one fixed order, no atomics: the same inputs give the same bits.
// A component of weight -inf is not read and gets gradient exactly zero; an empty group gives zeros; a NaN weight gives NaN
// for its group (in the shared form for every component of the row, which all groups share).
//   workgroup = 256 consecutive lanes; n is a run-time loop, p and s are unrolled over the instantiation's extent DP.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <2>      96      0        0             5
//   <4>     138      0        0             3
//   <8>     256     16        0             1
// No instantiation uses scratch; no LDS.
#include "switching_host.hpp"

namespace aesmc {

constexpr int kScbMaxComponents = 256;
constexpr int kScbMaxGroups = 256;

struct CollapseBackwardArgs {
  const double *mean, *cov, *log_weight;               // K50's inputs
  const double *grad_mass, *grad_mean_out, *grad_cov_out;      // [B,G], [B,G,D], [B,G,D(D+1)/2]
  double *grad_lw, *grad_mean, *grad_cov;              // [B,G,N]; [B,G,N,D] and [B,G,N,TD] (shared: [B,N,D], [B,N,TD]); may be NULL
  int64_t total;                                       // lanes: B G (dense), B (shared)
  int G, N, D, shared;
};

template <int DP> __global__ __launch_bounds__(kSkBlock) void switching_collapse_backward_kernel(const CollapseBackwardArgs a) {
  constexpr int TP = DP * (DP + 1) / 2;
  const int64_t lane = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (lane >= a.total) return;
  const int N = a.N, D = a.D, TD = D * (D + 1) / 2;
  const int groups = a.shared ? a.G : 1;
  const double ninf = Num<double>::neg_inf();
  for (int walk = 0; walk < groups; ++walk) {
    const int64_t group = a.shared ? lane * a.G + walk : lane;      // b G + g
    const int64_t block = a.shared ? lane : group;                  // the block of N components
    const bool adds = walk > 0;
    const double *lw = a.log_weight + group * N;
    const double *mean = a.mean + block * N * D, *cov = a.cov + block * N * TD;
    double *glw = a.grad_lw != nullptr ? a.grad_lw + group * N : nullptr;
    double *gmean = a.grad_mean != nullptr ? a.grad_mean + block * N * D : nullptr;
    double *gcov = a.grad_cov != nullptr ? a.grad_cov + block * N * TD : nullptr;
    const auto put = [&](double *at, double value) { *at = adds ? *at + value : value; };

    double top = ninf;
    bool bad = false;
    for (int n = 0; n < N; ++n) {
      const double w = lw[n];
      bad = bad || w != w;
      top = w > top ? w : top;
    }
    if (bad || top == ninf) {
      const double value = bad ? Num<double>::nan() : 0.0;
      for (int n = 0; n < N; ++n) {
        if (glw != nullptr) glw[n] = value;
        if (gmean != nullptr)
          for (int p = 0; p < D; ++p) put(gmean + (int64_t)n * D + p, value);
        if (gcov != nullptr)
          for (int e = 0; e < TD; ++e) put(gcov + (int64_t)n * TD + e, value);
      }
      continue;
    }
    double sum = 0.0;
    for (int n = 0; n < N; ++n) sum = sum + exp(lw[n] - top);
    const double scale = 1.0 / sum;
    double m[DP], mu[DP], c[TP];
    const double abar = a.grad_mass[group];
#pragma unroll
    for (int p = 0; p < DP; ++p) m[p] = 0.0, mu[p] = p < D ? a.grad_mean_out[group * D + p] : 0.0;
#pragma unroll
    for (int e = 0; e < TP; ++e) c[e] = e < TD ? a.grad_cov_out[group * TD + e] : 0.0;
    for (int n = 0; n < N; ++n) {
      const double l = lw[n];
      if (l == ninf) continue;
      const double w = exp(l - top) * scale;
      const double *row = mean + (int64_t)n * D;
#pragma unroll
      for (int p = 0; p < DP; ++p) m[p] = __builtin_fma(w, p < D ? row[p] : 0.0, m[p]);
    }
    // omega_n and their weighted mean
    const auto omega = [&](int n, double *d) {
      const double *row = mean + (int64_t)n * D, *prow = cov + (int64_t)n * TD;
      double acc = 0.0;
#pragma unroll
      for (int p = 0; p < DP; ++p) {
        d[p] = (p < D ? row[p] : 0.0) - m[p];
        acc = __builtin_fma(mu[p], d[p], acc);
      }
#pragma unroll
      for (int p = 0; p < DP; ++p) {
#pragma unroll
        for (int s = 0; s <= p; ++s) {
          const int e = sk_tri(p, s);
          acc = __builtin_fma(c[e], __builtin_fma(d[p], d[s], e < TD ? prow[e] : 0.0), acc);
        }
      }
      return acc;
    };
    double centre = 0.0;
    for (int n = 0; n < N; ++n) {
      const double l = lw[n];
      if (l == ninf) continue;
      double d[DP];
      centre = __builtin_fma(exp(l - top) * scale, omega(n, d), centre);
    }
    for (int n = 0; n < N; ++n) {
      const double l = lw[n];
      const bool dead = l == ninf;
      double d[DP];
      const double w = dead ? 0.0 : exp(l - top) * scale;
      const double om = dead ? 0.0 : omega(n, d);
      if (glw != nullptr) glw[n] = dead ? 0.0 : w * ((abar + om) - centre);
      if (gmean != nullptr) {
#pragma unroll
        for (int p = 0; p < DP; ++p) {
          double acc = mu[p];      // mu_p + 2 (sym(c) d)_p: the packed diagonal once, an off-diagonal element as it is
#pragma unroll
          for (int s = 0; s < DP; ++s) acc = __builtin_fma(p == s ? 2.0 * c[sk_tri(p, s)] : c[sk_tri(p, s)], dead ? 0.0 : d[s], acc);
          if (p < D) put(gmean + (int64_t)n * D + p, dead ? 0.0 : w * acc);
        }
      }
      if (gcov != nullptr) {
#pragma unroll
        for (int e = 0; e < TP; ++e)
          if (e < TD) put(gcov + (int64_t)n * TD + e, dead ? 0.0 : w * c[e]);
      }
    }
  }
}

}  // namespace aesmc

extern "C" int aesmc_switching_collapse_backward(const double *mean, int64_t mean_group_stride, const double *cov,
                                                 int64_t cov_group_stride, const double *log_weight, const double *grad_log_mass,
                                                 const double *grad_mean_out, const double *grad_cov_out,
                                                 double *grad_log_weight, double *grad_mean, double *grad_cov, int64_t B,
                                                 int64_t G, int64_t N, int64_t D, void *stream) {
  using namespace aesmc;
  if (mean == nullptr || cov == nullptr || log_weight == nullptr || grad_log_mass == nullptr || grad_mean_out == nullptr ||
      grad_cov_out == nullptr || B < 0 || G < 0 || N < 0 || D < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (grad_log_weight == nullptr && grad_mean == nullptr && grad_cov == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  const auto stride_fits = [&](int64_t stride, int64_t per) {
    if (stride == 0) return true;
    if (N > (1 << 20) || D > (1 << 20)) return stride > 0;
    return stride == N * per;
  };
  if (!stride_fits(mean_group_stride, D) || !stride_fits(cov_group_stride, D * (D + 1) / 2)) return AESMC_ERR_INVALID_ARGUMENT;
  // the two operands are shared together or not at all (N == 0: both strides are 0 either way)
  if ((mean_group_stride == 0) != (cov_group_stride == 0)) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(log_weight, 8) || !sk_aligned(grad_log_mass, 8) ||
      !sk_aligned(grad_mean_out, 8) || !sk_aligned(grad_cov_out, 8) || !sk_aligned(grad_log_weight, 8) ||
      !sk_aligned(grad_mean, 8) || !sk_aligned(grad_cov, 8))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({grad_log_weight, grad_mean, grad_cov},
                           {mean, cov, log_weight, grad_log_mass, grad_mean_out, grad_cov_out}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || G == 0) return AESMC_OK;
  if (D > kSkMaxDim || N > kScbMaxComponents || G > kScbMaxGroups || !sk_fits_32bit(B, G, 1)) return AESMC_ERR_UNSUPPORTED;
  CollapseBackwardArgs a;
  a.mean = mean, a.cov = cov, a.log_weight = log_weight;
  a.grad_mass = grad_log_mass, a.grad_mean_out = grad_mean_out, a.grad_cov_out = grad_cov_out;
  a.grad_lw = grad_log_weight, a.grad_mean = grad_mean, a.grad_cov = grad_cov;
  a.shared = mean_group_stride == 0 && N > 0 ? 1 : 0;
  a.total = a.shared ? B : B * G;
  a.G = (int)G, a.N = (int)N, a.D = (int)D;
  return sk_for_extent(sk_pad(D), [&](auto d) {
    return sk_launch(&switching_collapse_backward_kernel<decltype(d)::value>, sk_grid(a.total), dim3(kSkBlock), 0,
                     (hipStream_t)stream, a);
  });
}
