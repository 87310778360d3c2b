// K2's sibling: STRATIFIED ancestral resampling — one independent uniform per particle,
//   pos[k]   = min((u[b,k] + k) / K, 1 - 2^-53)        (float64: the sum, the true division, the clamp)
//   idx[b,k] = #{ j : c[j] <= pos[k] }
// over the same float64 CDF c as the systematic kernels of ancestor_index.hip (ancestor_index.hpp: exp_nonpositive, the
// blocked scan, division by the last entry through divide_with_reciprocal).  The reference resamples systematically only
// (aesmc/inference.py:234-269); this is the second scheme every particle-filter library offers.  It has exactly one
// position per stratum [k / K, (k + 1) / K], so the positions — and with them the ancestor indices — are non-decreasing
// along k: the sorted gather backward, the children ranges and the in-launch gathers downstream keep working unchanged.
//
// The clamp: u + (K - 1) can round up to K, i.e. to the position 1.0, which no particle's stratum holds; clamped to the
// largest float64 below 1 it selects the first particle whose CDF entry is 1.0 — one of positive weight — so a
// non-degenerate row never yields the index K.
//
// That one comparison — the CDF against 1.0 itself — is the only one whose answer depends on the ORDER of the sum: "the
// first entry that equals the total" moves with the association wherever the tail's weights sit at the rounding threshold
// of the total (a blocked scan adds several of them up before the total sees them; the contract's sequential sum drops
// them one by one), and behind the last non-zero weight two lanes hold the same sum one ulp apart.  Only the LAST position
// can reach the clamp's value ((u + k) / K <= (K - 1) / K for every other k), and only for u >= 1 - K 2^-53 — never with
// drawn uniforms.  A row that has it settles that one count in the contract's order: one lane adds the row's weights
// left to right and reports the last particle that still changed the sum; the inversion is told that exactly the
// particles before it are reached by the last position.  Every other comparison is a measure-zero knife edge, as in the
// systematic kernels.
//
// Two kernels, as for the systematic scheme, and built from the same phases (ancestor_index.hpp: row max, CDF, the tail
// from first[] to the indices, the stored CDF and its search); what is written here is what only this scheme has:
//   * ancestor_index_stratified_inv_kernel (K <= 32768, one workgroup per batch row): ancestor_index_inv_kernel's
//     structure — CDF entries in registers, inversion per SOURCE particle, int32 max-scan over the markers.  Only the
//     inversion differs: the positions are not an arithmetic progression, but pos[k] lies in stratum k, so the first
//     position that reaches c[j] is within one stratum of floor(c[j] K): it is settled against the exactly rounded
//     positions of the strata m - 1, m, m + 1 (three 8-byte reads of the row's uniforms, neighbours of the lane's last
//     ones: cache hits after the first) — no search;
//   * ancestor_index_stratified_kernel (larger K): ancestor_index_kernel's stored CDF (caller workspace) and its
//     galloping search per position, on the stratified positions.
#include "ancestor_index.hpp"

namespace aesmc {

// The largest float64 below 1.
__device__ __forceinline__ double below_one() { return 0x1.fffffffffffffp-1; }

// pos[k] of the contract, correctly rounded throughout (divide_with_reciprocal gives the true quotient's rounding).
__device__ __forceinline__ double stratified_position(double uk, int k, double dK, double inv_K) {
  return fmin(divide_with_reciprocal(uk + (double)k, dK, inv_K), below_one());
}

// #{ j : c[j] < 1 } in the contract's own order (see the top of the file): the index of the last particle whose weight
// still changes the left-to-right float64 sum — from it on every sequential partial sum equals the total.  One lane,
// K dependent additions: run only for a row whose last position sits at the clamp's value.
template <typename T> __device__ int sequential_top_count(const T *lw, int K, double dm) {
  double sum = 0.0;
  int last = 0;
  for (int j = 0; j < K; ++j) {
    const double next = sum + exp_nonpositive((double)lw[j] - dm);
    if (next != sum) last = j;
    sum = next;
  }
  return last;
}

template <typename T, int C>
__global__ __launch_bounds__(kMaxThreads) void ancestor_index_stratified_inv_kernel(
    const T *__restrict__ log_w, const double *__restrict__ u, int64_t *__restrict__ out_idx, int32_t *flags, int K,
    T *__restrict__ out_lse, int32_t *__restrict__ out_child_end) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *scratch = smem;                                        // [64]
  int *scratch_i = reinterpret_cast<int *>(scratch + 32);
  int *marker = reinterpret_cast<int *>(smem + kScratchDoubles);  // [K rounded up to C]
  const int tid = threadIdx.x;
  const int nt = blockDim.x;
  const int lane = tid % kWave;
  const int wave = tid / kWave;
  const int nwaves = nt / kWave;
  int *first_of_lane = marker + nt * C;                           // [nwaves]: first[] of each wavefront's lane 0; [16 + nwaves]: minima
  const int64_t row = blockIdx.x;
  const T *lw = log_w + row * (int64_t)K;
  const double *ur = u + row * (int64_t)K;
  int64_t *idx = out_idx + row * (int64_t)K;
  const int j0 = tid * C;                                         // nt * C >= K: one round

  // ---- load once, row max + NaN scan ---------------------------------------------------------
  T v[C];
  load_blocked<T, C>(lw, j0, K, v);
  T m;
  int has_nan;
  lane_max_nan<T, C>(v, m, has_nan);
  wave_max_nan(m, has_nan);
  if (lane == 0) {
    scratch[wave] = (double)m;
    scratch_i[wave] = has_nan;
  }
  __syncthreads();
  const RowMax all = collect_max_nan(scratch, scratch_i, nwaves);
  const double dm = all.dm;
  has_nan = all.has_nan;
  const bool degenerate = has_nan || !(dm > -__builtin_huge_val() && dm < __builtin_huge_val());
  if (degenerate) {  // same conventions as the systematic kernels: see include/aesmc_hip.h, K2
    if (tid == 0) {
      raise_flag(flags, has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
      // torch.logsumexp's values for such rows (K1 returns the same)
      if (out_lse != nullptr) out_lse[row] = has_nan ? Num<T>::nan() : (T)dm;
    }
    for (int i = 0; i < C; ++i)
      if (j0 + i < K) {
        idx[j0 + i] = (int64_t)K;
        if (out_child_end != nullptr) out_child_end[row * (int64_t)K + j0 + i] = 0;     // nobody has children
      }
    return;
  }

  // ---- float64 weights, blocked inclusive scan: the systematic kernels' CDF, bit for bit --------
  double s[C];
  const RowScan scan = blocked_cdf<T, C>(v, dm, j0, K, lane, wave, scratch, s);
  const double base = scan.base, total = scan.total;
  const double inv_total = 1.0 / total;
  // by-product: logsumexp of the row (the step's contribution to log Z), float64 inside
  if (out_lse != nullptr && tid == 0) out_lse[row] = (T)(dm + ::log(total));

  // ---- first[j] = min{ k : pos[k] >= c[j] }  (K when no position reaches c[j]) ----------------------------------------
  // pos[] is non-decreasing — fl(k / K) <= pos[k] <= fl((k + 1) / K), rounding being monotone — so the set is an upper
  // range of k and any starting point walks to its lower end.  Started from m = floor(c K): pos[m - 2] <= (m - 1) / K < c
  // and pos[m + 1] >= (m + 1) / K > c unless c K sits within rounding of an integer, so the three strata read up front
  // settle it; the loops behind them run only in that rare case (and bound a row of uniforms outside [0, 1)).
  const double dK = (double)K;
  const double inv_K = 1.0 / dK;
  int first[C];
#pragma unroll
  for (int i = 0; i < C; ++i) {
    if (j0 + i < K) {
      // (clamped as in the systematic kernels: a tree-ordered scan may leave an entry one ulp above the last one)
      const double c = fmin(divide_with_reciprocal(base + s[i], total, inv_total), 1.0);
      const double x = c * dK;
      int mid = x < dK ? (int)x : K - 1;                        // x >= 0: truncation is the floor
      mid = min(max(mid, 0), K - 1);                            // (every read below stays inside the row whatever x is)
      const int lo = mid > 0 ? mid - 1 : 0, hi = mid + 1 < K ? mid + 1 : K - 1;
      const double u_lo = ur[lo], u_mid = ur[mid], u_hi = ur[hi];
      const bool at_lo = mid > 0 && stratified_position(u_lo, lo, dK, inv_K) >= c;
      const bool at_mid = stratified_position(u_mid, mid, dK, inv_K) >= c;
      const bool at_hi = mid + 1 >= K || stratified_position(u_hi, hi, dK, inv_K) >= c;
      int k0;
      if (at_lo) {
        k0 = mid - 1;
        while (k0 > 0 && stratified_position(ur[k0 - 1], k0 - 1, dK, inv_K) >= c) --k0;
      } else if (at_mid) {
        k0 = mid;
      } else if (at_hi) {
        k0 = mid + 1;
      } else {
        k0 = mid + 2;
        while (k0 < K && stratified_position(ur[k0], k0, dK, inv_K) < c) ++k0;
      }
      first[i] = k0;
    } else {
      first[i] = K;
    }
  }
  // The last position at the clamp's value (row-uniform; never with drawn uniforms): which particles it reaches is the
  // comparison of the CDF with 1.0 itself — settled in the contract's order, see the top of the file.  Exactly the
  // particles before the last one that changes the sequential sum are reached by position K - 1, nobody later by any.
  if (stratified_position(ur[K - 1], K - 1, dK, inv_K) >= below_one()) {
    if (tid == 0) scratch_i[0] = sequential_top_count(lw, K, dm);      // (scratch_i: read last in front of the scan's barrier)
    __syncthreads();
    const int reached = scratch_i[0];
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (j0 + i < K) first[i] = j0 + i < reached ? min(first[i], K - 1) : K;
  }
  // ---- markers, max-scan, stores: idx[k] and the children ranges ---------------------------------
  int best[C];
  indices_from_first<C>(first, best, K, j0, lane, wave, nwaves, marker, first_of_lane, scratch_i, out_child_end, row, idx,
                        true);
}

// ---- the stored-CDF form (K > 32768): ancestor_index_kernel on the stratified positions ---------------------------------
template <typename T, int kChunk>
__global__ __launch_bounds__(kMaxThreads) void ancestor_index_stratified_kernel(
    const T *__restrict__ log_w, const double *__restrict__ u, int64_t *__restrict__ out_idx, int32_t *flags, int K,
    double *__restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *scratch = smem;
  double *cdf = ws + (size_t)blockIdx.x * (size_t)cdf_row_slots(K);   // this row's slice of the workspace

  const int tid = threadIdx.x;
  const int nt = blockDim.x;
  const int lane = tid % kWave;
  const int wave = tid / kWave;
  const int nwaves = nt / kWave;
  const int64_t row = blockIdx.x;
  const T *lw = log_w + row * (int64_t)K;
  const double *ur = u + row * (int64_t)K;
  int64_t *idx = out_idx + row * (int64_t)K;

  // ---- pass 1: row max, NaN detection ---------------------------------------------------------
  int *scratch_i = reinterpret_cast<int *>(scratch + 32);
  T m;
  int has_nan;
  strided_max_nan(lw, K, tid, nt, m, has_nan);
  wave_max_nan(m, has_nan);
  if (lane == 0) {
    scratch[wave] = (double)m;
    scratch_i[wave] = has_nan;
  }
  __syncthreads();
  const RowMax all = collect_max_nan(scratch, scratch_i, nwaves);
  const double dm = all.dm;
  has_nan = all.has_nan;
  __syncthreads();  // scratch is reused below

  const bool degenerate = has_nan || !(dm > -__builtin_huge_val() && dm < __builtin_huge_val());
  if (degenerate) {
    if (tid == 0) raise_flag(flags, has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
    for (int k = tid; k < K; k += nt) idx[k] = (int64_t)K;
    return;
  }

  // ---- passes 2, 3: the normalised float64 CDF, stored ------------------------------------------
  store_normalised_cdf<T, kChunk>(lw, K, dm, cdf, scratch, tid, nt, lane, wave, nwaves);
  // the last position at the clamp's value (row-uniform, never with drawn uniforms): its answer in the contract's order
  const double dK = (double)K;
  const double inv_K = 1.0 / dK;
  const bool top = stratified_position(ur[K - 1], K - 1, dK, inv_K) >= below_one();
  if (top && tid == 0) scratch_i[0] = sequential_top_count(lw, K, dm);      // (scratch_i: read last in front of pass 2)
  __syncthreads();

  // ---- pass 4: idx[k] = #{ j : c[j] <= pos[k] }; the last position at the clamp answers `reached` ----------------------
  const int reached = top ? scratch_i[0] : 0;
  search_stored_cdf<kChunk>(
      cdf, idx, K, tid, nt, [=](int k) { return stratified_position(ur[k < K ? k : K - 1], k, dK, inv_K); }, top, reached);
}

template <typename T, int C>
static int launch_stratified_inv(const void *log_w, const double *u, int64_t *idx, void *out_lse, int32_t *child_end,
                                 int32_t *flags, int64_t B, int64_t K, hipStream_t s) {
  const int nt = pick_threads(K, C);
  if (raise_dynamic_lds_cap<ancestor_index_stratified_inv_kernel<T, C>>() != AESMC_OK) return AESMC_ERR_LAUNCH;
  hipLaunchKernelGGL((ancestor_index_stratified_inv_kernel<T, C>), dim3((unsigned)B), dim3(nt), inv_lds_bytes(nt, C), s,
                     (const T *)log_w, u, idx, flags, (int)K, (T *)out_lse, child_end);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

// Four particles per lane up to 4096 (the systematic ladder stops them at 2048); beyond 32768 particles the CDF goes
// through the caller's workspace and the by-products are the host's to compose.
template <typename T>
static int launch_stratified(const void *log_w, const double *u, int64_t *idx, void *out_lse, int32_t *child_end,
                             int32_t *flags, int64_t B, int64_t K, void *ws, size_t ws_bytes, hipStream_t s) {
  if (K <= kInvMaxParticles)
    return launch_by_row_length(K, 4096, [&](auto c) {
      return launch_stratified_inv<T, decltype(c)::value>(log_w, u, idx, out_lse, child_end, flags, B, K, s);
    });
  if (out_lse != nullptr || child_end != nullptr) return AESMC_ERR_UNSUPPORTED;
  if (ws == nullptr || ws_bytes < aesmc_workspace_bytes(B, K)) return AESMC_ERR_WORKSPACE;
  const size_t lds = (size_t)kScratchDoubles * sizeof(double);
  hipLaunchKernelGGL((ancestor_index_stratified_kernel<T, 8>), dim3((unsigned)B), dim3(kMaxThreads), lds, s,
                     (const T *)log_w, u, idx, flags, (int)K, (double *)ws);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc

extern "C" int aesmc_resample_step_stratified(int dtype, const void *log_w, const double *u, int64_t *out_idx,
                                              void *out_lse, int32_t *out_child_end, int32_t *flags, int64_t B,
                                              int64_t K, void *ws, size_t ws_bytes, void *stream) {
  using namespace aesmc;
  if (log_w == nullptr || u == nullptr || out_idx == nullptr || B < 0 || K < 0 ||
      (((uintptr_t)out_child_end) & 3u) != 0 || (((uintptr_t)u) & 7u) != 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || K == 0) return AESMC_OK;
  if (K > 0x3fffffffLL || B > 0x7fffffffLL) return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_stratified<float>(log_w, u, out_idx, out_lse, out_child_end, flags, B, K, ws, ws_bytes, s);
  return launch_stratified<double>(log_w, u, out_idx, out_lse, out_child_end, flags, B, K, ws, ws_bytes, s);
}
