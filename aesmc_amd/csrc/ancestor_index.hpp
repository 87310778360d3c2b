// What the resampling kernels share (K2, systematic: ancestor_index.hip; its stratified sibling:
// ancestor_index_stratified.hip): the float64 CDF arithmetic — one definition, so that both schemes form a row's CDF
// with the same bits — the workgroup's LDS layout and the workspace layout of the stored-CDF form.
#pragma once
#include "common.hpp"

namespace aesmc {

constexpr int kMaxThreads = 1024;
constexpr int kScratchDoubles = 64;  // per-workgroup LDS scratch (wavefront totals, reduce slots)
constexpr int kScanSlot = 40;        // inv kernel: [0,16) maxima, [32,40) int flags / max-scan, [40,58) the scan's
// Stored-CDF kernel (K > 32768): the row's float64 CDF lives in the caller's workspace with one
// padding slot per 8 entries (lane t writes entries 8t..8t+7: a 72-byte lane stride keeps the
// lanes of a wavefront in different memory channels); aesmc_workspace_bytes accounts for the pad.
__host__ __device__ __forceinline__ int64_t cdf_slot(int64_t e) { return e + (e >> 3); }
__host__ __device__ __forceinline__ int64_t cdf_row_slots(int64_t K) { return cdf_slot(K) + 1; }

// exp(x) for x <= 0 in float64: Cody-Waite reduction x = n ln2 + r, |r| <= ln2 / 2, degree-13
// Taylor polynomial (truncation < 5e-18 relative), scaling by v_ldexp_f64.  exp(0) == 1 exactly.
__device__ __forceinline__ double exp_nonpositive(double x) {
  if (!(x > -745.2)) return 0.0;  // exp underflows to zero below ~ -745.13 (also catches -inf)
  const double n = __builtin_rint(x * 1.4426950408889634074);
  double r = __builtin_fma(-n, 6.93147180369123816490e-01, x);
  r = __builtin_fma(-n, 1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;               // 1/13!
  p = __builtin_fma(p, r, 2.08767569878681e-09);   // 1/12!
  p = __builtin_fma(p, r, 2.505210838544172e-08);  // 1/11!
  p = __builtin_fma(p, r, 2.755731922398589e-07);  // 1/10!
  p = __builtin_fma(p, r, 2.7557319223985893e-06); // 1/9!
  p = __builtin_fma(p, r, 2.48015873015873e-05);   // 1/8!
  p = __builtin_fma(p, r, 1.984126984126984e-04);  // 1/7!
  p = __builtin_fma(p, r, 1.3888888888888889e-03); // 1/6!
  p = __builtin_fma(p, r, 8.333333333333333e-03);  // 1/5!
  p = __builtin_fma(p, r, 4.1666666666666664e-02); // 1/4!
  p = __builtin_fma(p, r, 1.6666666666666666e-01); // 1/3!
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  return __builtin_ldexp(p, (int)n);
}

// a / b given y = 1 / b (a true, correctly rounded division done once per row): q0 = a y,
// r = a - b q0 (exact in an FMA), q = q0 + r y is the correctly rounded quotient.
__device__ __forceinline__ double divide_with_reciprocal(double a, double b, double y) {
  const double q0 = a * y;
  const double r = __builtin_fma(-b, q0, a);
  return __builtin_fma(r, y, q0);
}

// The in-workgroup kernels keep up to this many particles per lane: K <= 32768 in one workgroup.
constexpr int kInvMaxChunk = 32;
constexpr int64_t kInvMaxParticles = (int64_t)kMaxThreads * kInvMaxChunk;

// min over lanes >= this one of x (inclusive), by six bpermute steps: used only where the children ranges are written
// (training), to make them monotone on knife-edge rows — see the clamp in ancestor_index_inv_kernel.
__device__ __forceinline__ int wave_suffix_min(int x, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int other = __shfl_down(x, d, kWave);
    if (lane + d < kWave) x = min(x, other);
  }
  return x;
}

static inline int pick_threads(int64_t K, int chunk) {
  int64_t nt = (K + chunk - 1) / chunk;  // one round when it fits
  nt = (nt + kWave - 1) / kWave * kWave;
  if (nt < kWave) nt = kWave;
  if (nt > kMaxThreads) nt = kMaxThreads;
  return (int)nt;
}

}  // namespace aesmc
