// The host path of the switching linear-Gaussian kernels (switching_*.hip): the checks their C entries share, the dispatch
// over the padded extents and the launch.  Host code only — nothing here is compiled for the device, and no kernel's text
// depends on it.  An entry reads: its own checks, the shared ones, the argument structure, LDS bytes and grid, then
// sk_for_extents with a lambda that names the kernel.  Every check for AESMC_ERR_INVALID_ARGUMENT comes before the
// empty-launch return, every check for AESMC_ERR_UNSUPPORTED after it (tests/test_switching_abi_status.py).
#pragma once
#include <initializer_list>
#include <type_traits>

#include "switching_kalman.hpp"

namespace aesmc {

static inline bool sk_aligned(const void *p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
static inline int sk_pad(int64_t d) { return d <= 2 ? 2 : d <= 4 ? 4 : 8; }

// ---- AESMC_ERR_INVALID_ARGUMENT ------------------------------------------------------------------------------------------
static inline bool sk_extents_positive(int64_t M, int64_t D, int64_t Dy) { return M >= 1 && D >= 1 && Dy >= 1; }

// the operands every kernel stages (A, b, q, C, d, r) non-NULL and 8-aligned; `initial`: m0 and s0 as well (K34 and K36 do
// not read them).  The chain's rows are the entry's own business
static inline bool sk_model_operands(const aesmc_switching_model *model, bool initial) {
  const double *operands[] = {model->A, model->b, model->q, model->C, model->d, model->r, model->m0, model->s0};
  for (int i = 0; i < (initial ? 8 : 6); ++i)
    if (operands[i] == nullptr || !sk_aligned(operands[i], 8)) return false;
  return true;
}

// the observation: given, its dtype tag one of the two, aligned for it
static inline bool sk_observation(const void *y, int y_dtype) {
  return y != nullptr && (y_dtype == AESMC_F32 || y_dtype == AESMC_F64) && sk_aligned(y, y_dtype == AESMC_F32 ? 4 : 8);
}

static inline bool sk_among(const void *p, std::initializer_list<const void *> set) {
  for (const void *q : set)
    if (p == q) return true;
  return false;
}

// no output is an input or an earlier output (an output that is NULL is one the call does not ask for)
static inline bool sk_outputs_distinct(std::initializer_list<const void *> outputs, std::initializer_list<const void *> inputs) {
  for (const void *const *out = outputs.begin(); out != outputs.end(); ++out) {
    if (*out == nullptr) continue;
    if (sk_among(*out, inputs)) return false;
    for (const void *const *earlier = outputs.begin(); earlier != out; ++earlier)
      if (*out == *earlier) return false;
  }
  return true;
}

// ---- AESMC_ERR_UNSUPPORTED -------------------------------------------------------------------------------------------------
static inline bool sk_extents_supported(int64_t M, int64_t D, int64_t Dy) {
  return D <= kSkMaxDim && Dy <= kSkMaxDim && M <= kSkMaxRegimes;
}

// B x K rows of up to `elements` values each within 32-bit element arithmetic
constexpr int64_t kSkTriMax = kSkMaxDim * (kSkMaxDim + 1) / 2;      // a packed covariance at the largest D
static inline bool sk_fits_32bit(int64_t B, int64_t K, int64_t elements) {
  constexpr int64_t kLimit = 0x7fffffffLL;
  return B <= kLimit && K <= kLimit && B * K <= kLimit / elements;
}

// ---- the argument structure, the grid, the dispatch, the launch ----------------------------------------------------------------
template <typename Args> static inline void sk_fill_model(Args &a, const aesmc_switching_model *model) {
  a.A = model->A, a.b = model->b, a.q = model->q, a.C = model->C, a.d = model->d, a.r = model->r;
  a.M = (int)model->M, a.D = (int)model->D, a.Dy = (int)model->Dy;
}

static inline dim3 sk_grid(int64_t lanes) { return dim3((unsigned)((lanes + kSkBlock - 1) / kSkBlock)); }

// f(integral_constant<int, DP>) for a padded extent of sk_pad, and f(integral_constant<int, DP>, integral_constant<int, DYP>)
// for two: the instantiation is chosen here and nowhere else
template <typename F> static auto sk_for_extent(int dp, F f) {
  if (dp == 2) return f(std::integral_constant<int, 2>{});
  if (dp == 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}
template <typename F> static auto sk_for_extents(int dp, int dyp, F f) {
  return sk_for_extent(dp, [&](auto d) { return sk_for_extent(dyp, [&](auto dy) { return f(d, dy); }); });
}
// f(true_type) or f(false_type): a kernel's boolean parameter (Masked, Scores)
template <typename F> static auto sk_for_flag(bool flag, F f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }

// Enqueues `kernel` and returns the entry's status.  More than the default 64 KB of LDS (the 8-wide instantiations: 72 KB of
// covariances beside the model) need the limit raised; on every launch — no state to share between threads or devices, and
// the call is cheap beside the kernel.  The thread's last error is read, and so cleared, whatever happened before it
template <typename Args>
static int sk_launch(void (*kernel)(const Args), dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &a) {
  const void *handle = reinterpret_cast<const void *>(kernel);
  const bool raised = lds <= 64 * 1024 ||
                      hipFuncSetAttribute(handle, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  void *params[] = {const_cast<Args *>(&a)};
  const bool launched = raised && hipLaunchKernel(handle, grid, block, params, lds, s) == hipSuccess;
  return hipGetLastError() == hipSuccess && launched ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc
