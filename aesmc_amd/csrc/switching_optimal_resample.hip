// Optimal resampling for the discrete particle filter of a switching linear-Gaussian model (Fearnhead & Clifford 2003) —
// aesmc_switching_optimal_resample (K44) of include/aesmc_hip.h.  Every particle of a batch row proposes all M successor
// regimes with their exact weights (K43's scores); K_out of the K_in M candidates survive: whoever is heavier than the
// threshold c as it is, the rest thinned by ONE stratified draw to the weight c each.  No survivor appears twice.
//
//   workgroup = one batch row; 256 lanes up to 1024 candidates, 1024 lanes beyond; lanes stride over the candidates
//               (consecutive lanes on consecutive 8-byte words of LDS: no bank conflicts);
//   pass 1     a_i = log_w[k] + scores[k,j] from global memory, the row's maximum and NaN marker by the resampling kernels'
//              reduction (ancestor_index.hpp);
//   pass 2     e_i = exp_nonpositive(a_i - top) into LDS (0 below the smallest normal number: liveness must not hang on how
//              an exponential rounds a subnormal), their sum E, the number of live candidates and the first of them;
//   threshold  (only with more live candidates than slots) 62 rounds of a bisection over the order-preserving integer image
//              of e, one bit per round from the top: a round counts the candidates at or above the probe and reduces the
//              sum and the maximum of those below it; the probe stands where count >= K_out or max (K_out - count) < sum —
//              monotone in the probe in exact arithmetic, in floating point away from rounding of c (the contract's
//              weight margin); whatever rounds, the search ends on a probe that stands.  One barrier per round (the
//              wavefronts' partial results alternate between two sets of slots).  The largest probe that stands is the smallest kept weight; the last probe that fell gives the
//              count above it, which the cap L <= K_out - 1 needs where the stand is by count alone (ties are then kept
//              in ascending candidate order up to the cap);
//   scan       rounds of NT candidates: the kept ones' ranks by ballots, the not-kept weights' running sum Q by a scan that
//              adds front to back — inside a wavefront 64 steps of a broadcast and a predicated addition from zero, on
//              a base that is the chain of the earlier wavefronts' and rounds' totals — so that Q never decreases, a
//              wavefront's base is its predecessor's last entry and a candidate that adds nothing (kept, or of
//              weight 0) leaves it bit for bit: the intervals [Q_{i-1}, Q_i) tile [0, Q_last) exactly, whatever rounds.
//              Kept candidates are written to their slots here; Q replaces e in LDS;
//   draw       candidate i takes the slots L + n with Q_{i-1} <= position(n) < Q_i, n + u against t = R (Q / Q_last) in the
//              contract's own operations: every slot has exactly one writer.
//
// LDS: 8 bytes per candidate and 1280 bytes of reduction slots: 16384 candidates (aesmc_switching_optimal_resample_max_candidates)
// are 129.25 KB of the 160 KB.  No workspace, no atomics but the flags'.
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950):
//   <lanes>  VGPRs  AGPRs  scratch B/lane  waves/SIMD
//   <256>       54      0        0             7
//   <1024>      93      0        0             5       (16 wavefronts of a workgroup: 4 per SIMD)
#include "ancestor_index.hpp"
#include "switching_host.hpp"

namespace aesmc {

constexpr int64_t kOrMaxCandidates = 16384;
constexpr int kOrMaxWaves = 16;                               // 1024 lanes
constexpr double kOrLogMinNormal = -708.3964185322641;        // log(2^-1022)

struct OptimalResampleArgs {
  const double *log_w;      // [B,K_in] or NULL (zeros)
  const double *scores;     // [B,K_in,M]
  const double *u;          // [B]
  int64_t *parent;          // [B,K_out]
  int32_t *regime;          // [B,K_out]
  double *log_weight;       // [B,K_out]
  double *lse;              // [B]
  int32_t *count;           // [B]
  int32_t *flags;
  int K_in, M, K_out;
};

// what the wavefronts hand one another; [2]: alternating sets, so that a round needs one barrier
struct OrSlots {
  double sum[2][kOrMaxWaves], top[2][kOrMaxWaves];
  int count[2][kOrMaxWaves], first[kOrMaxWaves], nan[kOrMaxWaves];
  double q[2][kOrMaxWaves];
  int kept[2][kOrMaxWaves], ties[2][kOrMaxWaves];
};

static inline size_t or_lds_bytes(int64_t candidates) { return (size_t)candidates * sizeof(double) + sizeof(OrSlots); }

// sum over the wavefront, the same in every lane (xor butterfly)
__device__ __forceinline__ double or_wave_sum(double x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}
__device__ __forceinline__ int or_wave_sum(int x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// v_0 + v_1 + ... + v_lane, added one at a time in this order from v_0: never decreasing in the lane for v >= 0, and a lane
// that adds 0 holds its predecessor's bits
__device__ __forceinline__ double or_wave_running_sum(double v, int lane) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < kWave; ++s) {
    const double x = __hiloint2double(__builtin_amdgcn_readlane(hi, s), __builtin_amdgcn_readlane(lo, s));
    acc = lane >= s ? acc + x : acc;
  }
  return acc;
}

// #{ n in [0, R) : n + u < t }: the slots whose position lies below t, with the contract's own rounded n + u
__device__ __forceinline__ int or_slots_below(double t, double u, int R) {
  double guess = __builtin_ceil(t - u);
  guess = guess < 0.0 ? 0.0 : guess > (double)R ? (double)R : guess;
  int n = (int)guess;
  while (n > 0 && !((double)(n - 1) + u < t)) --n;
  while (n < R && (double)n + u < t) ++n;
  return n;
}

template <int NT>
__global__ __launch_bounds__(NT) void switching_optimal_resample_kernel(const OptimalResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) double or_smem[];
  constexpr int nwaves = NT / kWave;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int K_in = a.K_in, M = a.M, K_out = a.K_out;
  const int N = K_in * M;
  const int64_t b = blockIdx.x;
  double *e = or_smem;
  OrSlots *slots = reinterpret_cast<OrSlots *>(or_smem + N);
  const double *lw = a.log_w == nullptr ? nullptr : a.log_w + b * K_in;
  const double *sr = a.scores + b * N;
  int64_t *parent = a.parent + b * K_out;
  int32_t *regime = a.regime + b * K_out;
  double *out_lw = a.log_weight + b * K_out;
  const double inf = __builtin_huge_val(), nan = Num<double>::nan();
  auto candidate = [&](int i) { return lw == nullptr ? sr[i] : lw[i / M] + sr[i]; };

  // ---- pass 1: the maximum and the NaN marker ---------------------------------------------------------------------------
  double m = -inf;
  int has_nan = 0;
  for (int i = tid; i < N; i += NT) {
    const double x = candidate(i);
    has_nan |= (x != x);
    m = fmax(m, x);      // (fmax drops a NaN operand: the marker keeps it)
  }
  wave_max_nan<double>(m, has_nan);
  if (lane == 0) slots->top[0][wave] = m, slots->nan[wave] = has_nan;
  __syncthreads();
  const RowMax top = collect_max_nan(slots->top[0], slots->nan, nwaves);
  if (top.has_nan || !(fabs(top.dm) < inf)) {      // (workgroup-uniform) a bad row: the out-of-range marker and NaN
    if (tid == 0) {
      raise_flag(a.flags, top.has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
      a.lse[b] = nan;
      a.count[b] = 0;
    }
    for (int s = tid; s < K_out; s += NT) parent[s] = K_in, regime[s] = 0, out_lw[s] = nan;
    return;
  }

  // ---- pass 2: the weights into LDS, their sum, the live candidates ---------------------------------------------------
  double part = 0.0;
  int live = 0, first = N;
  for (int i = tid; i < N; i += NT) {
    const double x = candidate(i) - top.dm;
    const double w = x >= kOrLogMinNormal ? exp_nonpositive(x) : 0.0;
    e[i] = w;
    part += w;
    if (w > 0.0) {
      ++live;
      first = min(first, i);
    }
  }
  part = or_wave_sum(part);
  live = or_wave_sum(live);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, kWave));
  // (set 0 here, set 1 in the threshold's first round, bit 61: a wavefront that is ahead writes no slot another still reads)
  if (lane == 0) slots->sum[0][wave] = part, slots->count[0][wave] = live, slots->first[wave] = first;
  __syncthreads();
  double E = 0.0;
  int n_live = 0, first_live = N;
  for (int w = 0; w < nwaves; ++w) {
    E += slots->sum[0][w];
    n_live += slots->count[0][w];
    first_live = min(first_live, slots->first[w]);
  }
  const double lse = top.dm + ::log(E);
  const bool thin = n_live > K_out;      // (workgroup-uniform)

  // ---- the threshold: the largest probe that stands ---------------------------------------------------------------------
  unsigned long long cut = 1ull;      // without thinning: every live candidate is kept
  int above_cut = n_live, above_fallen = 0;
  if (thin) {
    cut = 0ull;
    for (int bit = 61; bit >= 0; --bit) {
      const unsigned long long probe = cut | (1ull << bit);
      const int set = bit & 1;
      int cnt = 0;
      double sum = 0.0, big = 0.0;
      for (int i = tid; i < N; i += NT) {
        const double w = e[i];
        if ((unsigned long long)__double_as_longlong(w) >= probe) {
          ++cnt;
        } else {
          sum += w;
          big = fmax(big, w);
        }
      }
      cnt = or_wave_sum(cnt);
      sum = or_wave_sum(sum);
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off, kWave));
      if (lane == 0) slots->count[set][wave] = cnt, slots->sum[set][wave] = sum, slots->top[set][wave] = big;
      __syncthreads();
      cnt = 0, sum = 0.0, big = 0.0;
      for (int w = 0; w < nwaves; ++w) {
        cnt += slots->count[set][w];
        sum += slots->sum[set][w];
        big = fmax(big, slots->top[set][w]);
      }
      if (cnt >= K_out || big * (double)(K_out - cnt) < sum) {
        cut = probe;
        above_cut = cnt;
      } else {
        above_fallen = cnt;
      }
    }
    __syncthreads();      // the last rounds' slots are read; the scan writes its own
  }
  // the cap L <= K_out - 1: of the candidates AT the cut only the first `quota` in ascending order are kept
  const bool capped = thin && above_cut >= K_out;
  const int quota = capped ? K_out - 1 - above_fallen : 0;

  // ---- the scan: kept candidates to their slots, the running sum of the others in place of e ------------------------------
  double q_carry = 0.0;
  int kept_carry = 0, tie_carry = 0, round = 0;
  for (int i0 = 0; i0 < N; i0 += NT, ++round) {
    const int set = round & 1;
    const int i = i0 + tid;
    const bool valid = i < N;
    const double w = valid ? e[i] : 0.0;
    const unsigned long long image = (unsigned long long)__double_as_longlong(w);
    const unsigned long long before = (1ull << lane) - 1ull;
    bool kept = valid && image >= cut;
    if (capped) {      // (workgroup-uniform)
      const bool tie = valid && image == cut;
      const unsigned long long ties = __ballot(tie);
      if (lane == 0) slots->ties[set][wave] = __popcll(ties);
      __syncthreads();
      int rank = tie_carry + __popcll(ties & before), all = tie_carry;
      for (int v = 0; v < nwaves; ++v) {
        if (v < wave) rank += slots->ties[set][v];
        all += slots->ties[set][v];
      }
      tie_carry = all;
      kept = valid && (image > cut || (tie && rank < quota));
    }
    const unsigned long long keeps = __ballot(kept);
    const double running = or_wave_running_sum(valid && !kept ? w : 0.0, lane);
    if (lane == kWave - 1) slots->q[set][wave] = running;
    if (lane == 0) slots->kept[set][wave] = __popcll(keeps);
    __syncthreads();
    double q_base = q_carry;
    int slot = kept_carry + __popcll(keeps & before);
    for (int v = 0; v < nwaves; ++v) {      // the totals in one chain: a wavefront's base is its predecessor's last entry
      if (v == wave) q_base = q_carry;
      if (v < wave) slot += slots->kept[set][v];
      q_carry += slots->q[set][v];
      kept_carry += slots->kept[set][v];
    }
    if (valid) e[i] = q_base + running;
    if (kept) {
      parent[slot] = i / M;
      regime[slot] = i % M;
      out_lw[slot] = candidate(i) - lse;
    }
  }
  __syncthreads();      // Q is complete
  const int L = kept_carry;      // (without thinning: n_live)
  if (tid == 0) {
    a.lse[b] = lse;
    a.count[b] = thin ? K_out : n_live;
  }
  if (!thin) {      // dead slots: slot 0's state, weight zero
    for (int s = L + tid; s < K_out; s += NT) parent[s] = first_live / M, regime[s] = first_live % M, out_lw[s] = -inf;
    return;
  }

  // ---- the stratified draw over the candidates that are not kept -------------------------------------------------------------
  const int R = K_out - L;
  const double q_last = q_carry, u = a.u[b];
  const double thinned = (top.dm + ::log(q_last / (double)R)) - lse;
  for (int i = tid; i < N; i += NT) {
    const double q = e[i], q_before = i > 0 ? e[i - 1] : 0.0;
    if (!(q > q_before)) continue;
    const int lo = or_slots_below((double)R * (q_before / q_last), u, R);
    const int hi = q == q_last ? R : or_slots_below((double)R * (q / q_last), u, R);
    for (int n = lo; n < hi; ++n) {
      parent[L + n] = i / M;
      regime[L + n] = i % M;
      out_lw[L + n] = thinned;
    }
  }
}

template <int NT> static int or_launch(int64_t B, size_t lds, hipStream_t s, const OptimalResampleArgs &a) {
  const int raised = raise_dynamic_lds_cap<switching_optimal_resample_kernel<NT>>();
  if (raised != AESMC_OK) return raised;
  hipLaunchKernelGGL((switching_optimal_resample_kernel<NT>), dim3((unsigned)B), dim3(NT), lds, s, a);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc

extern "C" int64_t aesmc_switching_optimal_resample_max_candidates(void) { return aesmc::kOrMaxCandidates; }

extern "C" int aesmc_switching_optimal_resample(const double *log_w, const double *scores, const double *u,
                                                int64_t *out_parent, int32_t *out_regime, double *out_log_weight,
                                                double *out_lse, int32_t *out_count, int32_t *flags, int64_t B, int64_t K_in,
                                                int64_t M, int64_t K_out, void *stream) {
  using namespace aesmc;
  if (scores == nullptr || u == nullptr || out_parent == nullptr || out_regime == nullptr || out_log_weight == nullptr ||
      out_lse == nullptr || out_count == nullptr || B < 0 || K_in < 0 || K_out < 0 || M < 1)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_aligned(log_w, 8) || !sk_aligned(scores, 8) || !sk_aligned(u, 8) || !sk_aligned(out_parent, 8) ||
      !sk_aligned(out_regime, 4) || !sk_aligned(out_log_weight, 8) || !sk_aligned(out_lse, 8) || !sk_aligned(out_count, 4) ||
      !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({out_parent, out_regime, out_log_weight, out_lse, out_count}, {log_w, scores, u, flags}))
    return AESMC_ERR_INVALID_ARGUMENT;      // an output that is an input, another output or the flags
  if (B == 0 || K_in == 0 || K_out == 0) return AESMC_OK;
  if (M > kSkMaxRegimes || K_in > kOrMaxCandidates || K_in * M > kOrMaxCandidates || !sk_fits_32bit(B, K_out, 1))
    return AESMC_ERR_UNSUPPORTED;
  OptimalResampleArgs a;
  a.log_w = log_w, a.scores = scores, a.u = u;
  a.parent = out_parent, a.regime = out_regime, a.log_weight = out_log_weight, a.lse = out_lse, a.count = out_count;
  a.flags = flags;
  a.K_in = (int)K_in, a.M = (int)M, a.K_out = (int)K_out;
  const size_t lds = or_lds_bytes(K_in * M);
  hipStream_t s = (hipStream_t)stream;
  return K_in * M <= 1024 ? or_launch<256>(B, lds, s, a) : or_launch<1024>(B, lds, s, a);
}
