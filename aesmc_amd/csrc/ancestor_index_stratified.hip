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
// Two kernels, as for the systematic scheme:
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
  constexpr int NV = Vec16<T>::N;
  if (C % NV == 0 && j0 + C <= K && (((uintptr_t)(lw + j0)) & 15u) == 0) {
    using V = typename Vec16<T>::type;                       // the lane's C values as 16-byte loads
#pragma unroll
    for (int q = 0; q < C / NV; ++q) {
      const V packed = reinterpret_cast<const V *>(lw + j0)[q];
#pragma unroll
      for (int r = 0; r < NV; ++r) v[q * NV + r] = Vec16<T>::get(packed, r);
    }
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i) v[i] = (j0 + i < K) ? lw[j0 + i] : Num<T>::neg_inf();
  }
  T m = Num<T>::neg_inf();
  int has_nan = 0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    has_nan |= (v[i] != v[i]);
    m = Num<T>::max(m, v[i]);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    m = Num<T>::max(m, __shfl_xor(m, off, kWave));
    has_nan |= __shfl_xor(has_nan, off, kWave);
  }
  if (lane == 0) {
    scratch[wave] = (double)m;
    scratch_i[wave] = has_nan;
  }
  __syncthreads();
  double dm = scratch[0];
  has_nan = scratch_i[0];
  for (int w = 1; w < nwaves; ++w) {
    dm = fmax(dm, scratch[w]);
    has_nan |= scratch_i[w];
  }
  // (no barrier here: the scan below publishes into scratch slots of its own, kScanSlot onwards)
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

  // ---- float64 weights, blocked inclusive scan: ancestor_index_inv_kernel's, operation for operation --------------
  double s[C];
  double run = 0.0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    run += (j0 + i < K) ? exp_nonpositive((double)v[i] - dm) : 0.0;
    s[i] = run;
  }
  double incl = run;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double y = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += y;
  }
  double base = __shfl_up(incl, 1, kWave);
  if (lane == 0) base = 0.0;
  double *scan = scratch + kScanSlot;                          // [16] wavefront totals, [16] / [17]: see below
  if (lane == kWave - 1) scan[wave] = incl;
  // The CDF's last entry is the normaliser, so that c[K-1] == 1.0 exactly: its owner publishes the two terms only it
  // has, and every lane adds the earlier wavefronts' totals in the owner's own order (see ancestor_index_inv_kernel).
  const int last_wave = ((K - 1) / C) / kWave;
  if (j0 <= K - 1 && K - 1 < j0 + C) {
    scan[16] = base;
    scan[17] = s[K - 1 - j0];
  }
  __syncthreads();
  for (int w = 0; w < wave; ++w) base += scan[w];
  double total = scan[16];
  for (int w = 0; w < last_wave; ++w) total += scan[w];
  total += scan[17];
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
  if (lane == 0) first_of_lane[wave] = first[0];            // the next wavefront's first entry, via LDS
  int wave_min = K;
  if (out_child_end != nullptr) {                           // (each wavefront's smallest first entry: see the clamp below)
    wave_min = wave_suffix_min(first[0], lane);             // min over lanes >= this one, this wavefront
    if (lane == 0) first_of_lane[16 + wave] = wave_min;
  }
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) reinterpret_cast<int4 *>(marker + j0)[q] = make_int4(0, 0, 0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i) marker[j0 + i] = 0;
  }
  __syncthreads();
  int next_lane_first = __shfl_down(first[0], 1, kWave);     // the next lane's first entry, in-register
  if (lane == kWave - 1) next_lane_first = (wave + 1 < nwaves) ? first_of_lane[wave + 1] : K;
  if (out_child_end != nullptr) {
    // The children ranges must be monotone; across lanes first[] can descend by one on a knife-edge position (two lanes
    // holding the same partial sum associated differently: ancestor_index_inv_kernel says how).  The indices the markers
    // produce are those of first[]'s SUFFIX MINIMUM; the ranges are made to say the same.
    int bound = __shfl_down(wave_min, 1, kWave);                       // min over the lanes BEHIND this one
    if (lane == kWave - 1) bound = K;
    for (int w = wave + 1; w < nwaves; ++w) bound = min(bound, first_of_lane[16 + w]);
#pragma unroll
    for (int i = 0; i < C; ++i) first[i] = min(first[i], bound);
    next_lane_first = min(next_lane_first, bound);
    // first[j] = how many positions precede the CDF at j = where the children of particles 0..j end
    int32_t *ends = out_child_end + row * (int64_t)K + j0;
    if (C % 4 == 0 && (K & 3) == 0 && j0 + C <= K && (reinterpret_cast<uintptr_t>(out_child_end) & 15u) == 0) {
#pragma unroll
      for (int q = 0; q < C / 4; ++q)
        reinterpret_cast<int4 *>(ends)[q] = make_int4(first[4 * q], first[4 * q + 1], first[4 * q + 2], first[4 * q + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < C; ++i)
        if (j0 + i < K) ends[i] = first[i];
    }
  }
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const int j = j0 + i;
    if (j < K) {
      int next = (i + 1 < C) ? first[i + 1 < C ? i + 1 : i] : next_lane_first;
      if (j == K - 1) next = K;
      if (first[i] < next) marker[first[i]] = j + 1;       // distinct j write distinct slots; first[i] < next <= K
    }
  }
  __syncthreads();

  // ---- idx[k] = running maximum of the markers ------------------------------------------------
  int best[C];
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
      const int4 packed = reinterpret_cast<const int4 *>(marker + j0)[q];
      best[4 * q] = packed.x;
      best[4 * q + 1] = packed.y;
      best[4 * q + 2] = packed.z;
      best[4 * q + 3] = packed.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i) best[i] = marker[j0 + i];
  }
  int acc = 0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    acc = max(acc, best[i]);
    best[i] = acc;
  }
  int incl_max = acc;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int y = __shfl_up(incl_max, off, kWave);
    if (lane >= off) incl_max = max(incl_max, y);
  }
  int before = __shfl_up(incl_max, 1, kWave);
  if (lane == 0) before = 0;
  if (lane == kWave - 1) scratch_i[wave] = incl_max;
  __syncthreads();
  for (int w = 0; w < wave; ++w) before = max(before, scratch_i[w]);
#pragma unroll
  for (int i = 0; i < C; ++i) best[i] = max(before, best[i]);
  if (j0 + C <= K && (((uintptr_t)(idx + j0)) & 15u) == 0) {
#pragma unroll
    for (int i = 0; i < C; i += 2) {
      longlong2 pair;
      pair.x = (int64_t)best[i];
      pair.y = (int64_t)best[i + 1];
      *reinterpret_cast<longlong2 *>(idx + j0 + i) = pair;
    }
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (j0 + i < K) idx[j0 + i] = (int64_t)best[i];
  }
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
  T m = Num<T>::neg_inf();
  int has_nan = 0;
  for (int k = tid; k < K; k += nt) {
    T v = lw[k];
    has_nan |= (v != v);
    m = Num<T>::max(m, v);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    m = Num<T>::max(m, __shfl_xor(m, off, kWave));
    has_nan |= __shfl_xor(has_nan, off, kWave);
  }
  int *scratch_i = reinterpret_cast<int *>(scratch + 32);
  if (lane == 0) {
    scratch[wave] = (double)m;
    scratch_i[wave] = has_nan;
  }
  __syncthreads();
  double dm = scratch[0];
  has_nan = scratch_i[0];
  for (int w = 1; w < nwaves; ++w) {
    dm = fmax(dm, scratch[w]);
    has_nan |= scratch_i[w];
  }
  __syncthreads();  // scratch is reused below

  const bool degenerate = has_nan || !(dm > -__builtin_huge_val() && dm < __builtin_huge_val());
  if (degenerate) {
    if (tid == 0) raise_flag(flags, has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
    for (int k = tid; k < K; k += nt) idx[k] = (int64_t)K;
    return;
  }

  // ---- pass 2: float64 weights, blocked scan (round r covers nt * kChunk particles; `carry`: the earlier rounds) ----
  const int per_round = nt * kChunk;
  double carry = 0.0;
  for (int round_base = 0; round_base < K; round_base += per_round) {
    const int first = round_base + tid * kChunk;
    double s[kChunk];
    double run = 0.0;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int k = first + i;
      run += (k < K) ? exp_nonpositive((double)lw[k < K ? k : 0] - dm) : 0.0;
      s[i] = run;
    }
    double incl = run;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const double y = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += y;
    }
    double excl = __shfl_up(incl, 1, kWave);  // exclusive prefix of this lane inside its wavefront
    if (lane == 0) excl = 0.0;
    if (lane == kWave - 1) scratch[wave] = incl;
    __syncthreads();
    double base = carry, round_total = 0.0;
    for (int w = 0; w < nwaves; ++w) {
      if (w == wave) base = carry + round_total;
      round_total += scratch[w];
    }
    base += excl;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int k = first + i;
      if (k < K) cdf[cdf_slot(k)] = base + s[i];
    }
    carry += round_total;
    __syncthreads();  // scratch is rewritten by the next round
  }

  // ---- pass 3: normalise by the row's last entry (every lane rereads only what it wrote) -------------
  __syncthreads();
  const double total = cdf[cdf_slot(K - 1)];
  __syncthreads();
  const double inv_total = 1.0 / total;
  for (int round_base = 0; round_base < K; round_base += per_round) {
    const int first = round_base + tid * kChunk;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int k = first + i;
      if (k < K) cdf[cdf_slot(k)] = divide_with_reciprocal(cdf[cdf_slot(k)], total, inv_total);
    }
  }
  // the last position at the clamp's value (row-uniform, never with drawn uniforms): its answer in the contract's order
  const double dK = (double)K;
  const double inv_K = 1.0 / dK;
  const bool top = stratified_position(ur[K - 1], K - 1, dK, inv_K) >= below_one();
  if (top && tid == 0) scratch_i[0] = sequential_top_count(lw, K, dm);      // (scratch_i: read last in front of pass 2)
  __syncthreads();

  // ---- pass 4: idx[k] = #{ j : c[j] <= pos[k] }; pos[] is non-decreasing, so each search gallops from the last ------
  const int reached = top ? scratch_i[0] : 0;
  for (int round_base = 0; round_base < K; round_base += per_round) {
    const int first = round_base + tid * kChunk;
    if (first >= K) break;
    int64_t found[kChunk];
    int answer = 0;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int k = first + i;
      const double pos = stratified_position(ur[k < K ? k : K - 1], k, dK, inv_K);
      int left, right;
      if (i == 0) {
        left = 0;
        right = K;
      } else {  // gallop from the previous particle's answer
        left = answer;
        int probe = answer, step = 1;
        while (probe < K && cdf[cdf_slot(probe)] <= pos) {
          left = probe + 1;
          probe += step;
          step <<= 1;
        }
        right = probe < K ? probe : K;
      }
      while (left < right) {
        const int mid = (left + right) >> 1;
        if (cdf[cdf_slot(mid)] <= pos)
          left = mid + 1;
        else
          right = mid;
      }
      answer = left;
      found[i] = (int64_t)((top && k == K - 1) ? reached : left);
    }
    if (first + kChunk <= K && (((uintptr_t)(idx + first)) & 15u) == 0) {
#pragma unroll
      for (int i = 0; i < kChunk; i += 2) {
        longlong2 pair;
        pair.x = found[i];
        pair.y = found[i + 1];
        *reinterpret_cast<longlong2 *>(idx + first + i) = pair;
      }
    } else {
#pragma unroll
      for (int i = 0; i < kChunk; ++i)
        if (first + i < K) idx[first + i] = found[i];
    }
  }
}

template <typename T, int C>
static int launch_stratified_inv(const void *log_w, const double *u, int64_t *idx, void *out_lse, int32_t *child_end,
                                 int32_t *flags, int64_t B, int64_t K, hipStream_t s) {
  const int nt = pick_threads(K, C);
  const size_t lds = (size_t)kScratchDoubles * sizeof(double) + (size_t)(nt * C + nt + 8) * sizeof(int);
  // raise the dynamic-LDS cap once per device and instantiation (a process may drive several GPUs)
  static bool attr_set[64] = {};
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= 64) return AESMC_ERR_LAUNCH;
  if (!attr_set[device]) {
    if (hipFuncSetAttribute((const void *)ancestor_index_stratified_inv_kernel<T, C>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return AESMC_ERR_LAUNCH;
    attr_set[device] = true;
  }
  hipLaunchKernelGGL((ancestor_index_stratified_inv_kernel<T, C>), dim3((unsigned)B), dim3(nt), lds, s,
                     (const T *)log_w, u, idx, flags, (int)K, (T *)out_lse, child_end);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

// Particles per lane grow with the row so that one workgroup (<= 1024 lanes) covers it, as for the systematic kernels;
// beyond 32768 particles the CDF goes through the caller's workspace and the by-products are the host's to compose.
template <typename T>
static int launch_stratified(const void *log_w, const double *u, int64_t *idx, void *out_lse, int32_t *child_end,
                             int32_t *flags, int64_t B, int64_t K, void *ws, size_t ws_bytes, hipStream_t s) {
  if (K <= 512) return launch_stratified_inv<T, 2>(log_w, u, idx, out_lse, child_end, flags, B, K, s);
  if (K <= 4096) return launch_stratified_inv<T, 4>(log_w, u, idx, out_lse, child_end, flags, B, K, s);
  if (K <= 8192) return launch_stratified_inv<T, 8>(log_w, u, idx, out_lse, child_end, flags, B, K, s);
  if (K <= 16384) return launch_stratified_inv<T, 16>(log_w, u, idx, out_lse, child_end, flags, B, K, s);
  if (K <= kInvMaxParticles) return launch_stratified_inv<T, 32>(log_w, u, idx, out_lse, child_end, flags, B, K, s);
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
