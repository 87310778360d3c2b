// What the resampling kernels share (K2, systematic: ancestor_index.hip; its stratified sibling:
// ancestor_index_stratified.hip): every phase that both schemes run has its ONE definition here, so that both form a
// row's CDF with the same bits and turn first[] into indices by the same steps —
//   the float64 arithmetic (exp_nonpositive, divide_with_reciprocal), the wavefront scans, the row max + NaN reduction and
//   its two loaders, the blocked in-register CDF, the tail from first[] to the indices (in-workgroup kernels), the stored
//   CDF and its galloping search (K > 32768), the workgroup's LDS layout, the workspace layout, and the host side's
//   launch helpers (dynamic-LDS cap, LDS size, particles-per-lane ladder).
// A scheme's own file keeps what only it has: how first[] is computed, its degenerate-row exit, its positions.
// (The lean DPP form of the systematic scheme, ancestor_index_rows_kernel, is written for the instruction count and
// shares only the arithmetic and wave_suffix_min.)
#pragma once
#include <type_traits>

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

// ---- wavefront scans (Hillis-Steele over 64 lanes; the order of the additions decides a CDF entry's last bit) ----------
__device__ __forceinline__ double wave_inclusive_add(double incl, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double y = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += y;
  }
  return incl;
}
__device__ __forceinline__ int wave_inclusive_max(int incl, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int y = __shfl_up(incl, off, kWave);
    if (lane >= off) incl = max(incl, y);
  }
  return incl;
}

// ---- row max + NaN detection ------------------------------------------------------------------------------------------
// In order: a loader leaves the lane's maximum and whether it met a NaN in (m, has_nan); wave_max_nan spreads them over the
// wavefront; lane 0 of each wavefront publishes them to scratch[wave] / scratch_i[wave] in front of one barrier; and
// collect_max_nan reads the workgroup's back.  The publish — two stores and the barrier — is written out in each kernel:
// as a function it cost the instantiations held to 64 registers another four bytes of scratch each.

// Loader of the in-workgroup kernels: the lane's C consecutive values (16-byte loads where the piece is whole and aligned;
// -inf beyond the row) ...
template <typename T, int C> __device__ __forceinline__ void load_blocked(const T *lw, int j0, int K, T (&v)[C]) {
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
}
// ... and what they hold.
template <typename T, int C> __device__ __forceinline__ void lane_max_nan(const T (&v)[C], T &m, int &has_nan) {
  m = Num<T>::neg_inf();
  has_nan = 0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    has_nan |= (v[i] != v[i]);
    m = Num<T>::max(m, v[i]);
  }
}

// Loader of the stored-CDF kernels: a strided pass over the row, nothing kept.
template <typename T>
__device__ __forceinline__ void strided_max_nan(const T *lw, int K, int tid, int nt, T &m, int &has_nan) {
  m = Num<T>::neg_inf();
  has_nan = 0;
  for (int k = tid; k < K; k += nt) {
    T v = lw[k];
    has_nan |= (v != v);
    m = Num<T>::max(m, v);
  }
}

template <typename T> __device__ __forceinline__ void wave_max_nan(T &m, int &has_nan) {      // xor butterfly: every lane
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    m = Num<T>::max(m, __shfl_xor(m, off, kWave));
    has_nan |= __shfl_xor(has_nan, off, kWave);
  }
}

// The whole row's, the same in every lane, from scratch[0, nwaves) / scratch_i[0, nwaves).  No barrier behind the reads:
// the in-workgroup kernels' scan publishes into scratch slots of its own (kScanSlot onwards); a caller that reuses the
// slots adds one.  A row with a NaN or without a finite maximum is degenerate: each kernel leaves by an exit of its own.
struct RowMax {
  double dm;
  int has_nan;
};
__device__ __forceinline__ RowMax collect_max_nan(const double *scratch, const int *scratch_i, int nwaves) {
  RowMax all = {scratch[0], scratch_i[0]};
  for (int w = 1; w < nwaves; ++w) {
    all.dm = fmax(all.dm, scratch[w]);
    all.has_nan |= scratch_i[w];
  }
  return all;
}

// ---- the blocked in-register CDF (in-workgroup kernels) -----------------------------------------------------------------
// s[i]: the lane's running sum of float64 weights exp(v - dm) up to its particle i; `base`: everything before the lane
// (its wavefront's earlier lanes, then the earlier wavefronts' totals in ascending order); `total`: the row's normaliser.
// The CDF entry of particle j0 + i is (base + s[i]) / total.  One barrier.
//
// The CDF's last entry is the normaliser, so that c[K-1] == 1.0 exactly (reference: c / max(c)).  Its owner publishes the
// two terms only it has — its exclusive prefix inside the wavefront and its running sum up to particle K - 1 — BEFORE the
// barrier (scan[16], scan[17]); every lane then adds the earlier wavefronts' totals in the owner's own order: the same
// value bit for bit, one barrier fewer.
struct RowScan {
  double base, total;
};
template <typename T, int C>
__device__ __forceinline__ RowScan blocked_cdf(const T (&v)[C], double dm, int j0, int K, int lane, int wave,
                                               double *scratch, double (&s)[C]) {
  double run = 0.0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    run += (j0 + i < K) ? exp_nonpositive((double)v[i] - dm) : 0.0;
    s[i] = run;
  }
  const double incl = wave_inclusive_add(run, lane);
  double base = __shfl_up(incl, 1, kWave);
  if (lane == 0) base = 0.0;
  double *scan = scratch + kScanSlot;                          // [16] wavefront totals, [16] / [17]: the owner's terms
  if (lane == kWave - 1) scan[wave] = incl;
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
  return {base, total};
}

// ---- the tail of the in-workgroup kernels: from first[] to the indices ---------------------------------------------------
// first[i] = the first position that reaches the CDF at particle j0 + i (K: none does; K too beyond the row).  Since
// idx[k] = #{ j : first[j] <= k }, lane j drops the marker j + 1 at k = first[j] (when any particle starts there) into
// LDS, and an inclusive max-scan over k — the same blocked scan as for the CDF, on int32 — turns the markers into the
// ancestor indices.  Three barriers.  `owns_idx`: whether this lane stores its indices and ranges (a batch row shared by
// several workgroups).  best[] returns the lane's C indices (the fused step copies the payload with them).
//
// out_child_end (may be null), the by-product for the gather's backward: first[j] = how many positions precede the CDF at
// j = where the children of particles 0..j end, so the children of particle j are the positions [first[j-1], first[j]) —
// one run, because the indices are non-decreasing (aesmc_affine_step_backward_resampled sums a particle's children with
// it).  The ranges must be monotone.  Within a lane first[] is (the lane's running sum is sequential); ACROSS lanes the
// CDF is assembled from tree-ordered partial sums, and where the weights in between underflow to exact zeros two lanes
// hold the same sum associated differently — one ulp apart in either order — so on a knife-edge position a later lane's
// first[] can come out one BELOW an earlier lane's.  The indices the markers produce are then the running maximum's, i.e.
// those of the SUFFIX MINIMUM of first[]; the ranges are made to say the same: every entry is clamped to the smallest
// first[] of all later lanes (a reverse scan over each lane's first entry: six bpermutes inside the wavefront, the later
// wavefronts' minima through LDS).
template <int C>
__device__ __forceinline__ void indices_from_first(int (&first)[C], int (&best)[C], int K, int j0, int lane, int wave,
                                                   int nwaves, int *marker, int *first_of_lane, int *scratch_i,
                                                   int32_t *out_child_end, int64_t row, int64_t *idx, bool owns_idx) {
  if (lane == 0) first_of_lane[wave] = first[0];            // the next wavefront's first entry, via LDS
  int wave_min = K;
  if (out_child_end != nullptr) {                           // (each wavefront's smallest first entry: for the clamp)
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
    int bound = __shfl_down(wave_min, 1, kWave);                       // min over the lanes BEHIND this one
    if (lane == kWave - 1) bound = K;
    for (int w = wave + 1; w < nwaves; ++w) bound = min(bound, first_of_lane[16 + w]);
#pragma unroll
    for (int i = 0; i < C; ++i) first[i] = min(first[i], bound);
    next_lane_first = min(next_lane_first, bound);
  }
  if (out_child_end != nullptr && owns_idx) {
    int32_t *ends = out_child_end + row * (int64_t)K + j0;
    // a lane's C entries are consecutive: whole 16-byte stores where the row allows (K a multiple of 4 keeps every
    // lane's first entry on a 16-byte boundary), else entry by entry
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

  // idx[k] = running maximum of the markers
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
  const int incl_max = wave_inclusive_max(acc, lane);
  int before = __shfl_up(incl_max, 1, kWave);
  if (lane == 0) before = 0;
  if (lane == kWave - 1) scratch_i[wave] = incl_max;      // (the NaN flags in these slots were read two barriers ago)
  __syncthreads();
  for (int w = 0; w < wave; ++w) before = max(before, scratch_i[w]);
#pragma unroll
  for (int i = 0; i < C; ++i) best[i] = max(before, best[i]);
  if (!owns_idx) {
    // another workgroup of this row stores these indices
  } else if (j0 + C <= K && (((uintptr_t)(idx + j0)) & 15u) == 0) {
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

// ---- the stored-CDF kernels (K > 32768) ---------------------------------------------------------------------------------
// Passes 2 and 3: the row's normalised float64 CDF into its padded workspace slice.  Round r covers particles
// [r * nt * kChunk, (r + 1) * nt * kChunk); lane `tid` owns kChunk consecutive ones; `carry` is the sum of all earlier
// rounds.  The last particle's CDF entry was formed by exactly the additions that formed `carry`'s summands in a
// different association; dividing by that entry itself keeps c[K-1] == 1.0.  Every lane rereads only what it wrote; the
// caller puts a barrier between this and the search.
template <typename T, int kChunk>
__device__ __forceinline__ void store_normalised_cdf(const T *lw, int K, double dm, double *cdf, double *scratch, int tid,
                                                     int nt, int lane, int wave, int nwaves) {
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
    const double incl = wave_inclusive_add(run, lane);
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
}

// Pass 4: idx[k] = #{ j : c[j] <= pos(k) } for non-decreasing positions: each search gallops from the previous
// particle's answer, then bisects.  `override_last`: particle K - 1 answers `last_answer` instead (stratified: the last
// position at the clamp's value); its search still runs.
template <int kChunk, typename Pos>
__device__ __forceinline__ void search_stored_cdf(const double *cdf, int64_t *idx, int K, int tid, int nt, Pos pos_of,
                                                  bool override_last, int last_answer) {
  const int per_round = nt * kChunk;
  for (int round_base = 0; round_base < K; round_base += per_round) {
    const int first = round_base + tid * kChunk;
    if (first >= K) break;
    int64_t found[kChunk];
    int answer = 0;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int k = first + i;
      const double pos = pos_of(k);
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
      found[i] = (int64_t)((override_last && k == K - 1) ? last_answer : left);
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

// ---- the host side of a launch --------------------------------------------------------------------------------------------
static inline int pick_threads(int64_t K, int chunk) {
  int64_t nt = (K + chunk - 1) / chunk;  // one round when it fits
  nt = (nt + kWave - 1) / kWave * kWave;
  if (nt < kWave) nt = kWave;
  if (nt > kMaxThreads) nt = kMaxThreads;
  return (int)nt;
}

// LDS of an in-workgroup kernel: the scratch, a marker per particle slot, first_of_lane ([nwaves] and [16 + nwaves])
static inline size_t inv_lds_bytes(int nt, int C) {
  return (size_t)kScratchDoubles * sizeof(double) + (size_t)(nt * C + nt + 8) * sizeof(int);
}

// Raise kernel kKernel's dynamic-LDS cap, once per device (a process may drive several GPUs).
template <auto kKernel> static int raise_dynamic_lds_cap() {
  static bool attr_set[64] = {};
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= 64) return AESMC_ERR_LAUNCH;
  if (!attr_set[device]) {
    if (hipFuncSetAttribute((const void *)kKernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return AESMC_ERR_LAUNCH;
    attr_set[device] = true;
  }
  return AESMC_OK;
}

// Particles per lane grow with the row so that one workgroup (<= 1024 lanes) covers it: launch_c(constant C) for a row of
// K <= kInvMaxParticles.  How far four per lane reach is the scheme's (and the launch's) own threshold.
template <typename LaunchC> static int launch_by_row_length(int64_t K, int64_t four_per_lane_max, LaunchC launch_c) {
  if (K <= 512) return launch_c(std::integral_constant<int, 2>{});
  if (K <= four_per_lane_max) return launch_c(std::integral_constant<int, 4>{});
  if (K <= 8192) return launch_c(std::integral_constant<int, 8>{});
  if (K <= 16384) return launch_c(std::integral_constant<int, 16>{});
  if (K <= kInvMaxParticles) return launch_c(std::integral_constant<int, 32>{});
  return AESMC_ERR_UNSUPPORTED;
}

}  // namespace aesmc
