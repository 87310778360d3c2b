// Backward simulation (FFBS, Godsill, Doucet & West 2004): one backward step for M trajectories per batch row —
// aesmc_backward_sample of include/aesmc_hip.h.  A pairwise (trajectory x particle) score with one categorical draw per
// trajectory, O(B M K D) and no [M,K] storage:
//
//   workgroup = (batch row b, tile of kTile trajectories); the tile's target rows and the reciprocal scales sit in LDS
//               as float64 (every lane reads the same address: a broadcast), read once from memory;
//   lanes     = particles: a wavefront walks whole CHUNKS of particles (runs of L, a multiple of 64, at most kMaxChunks of
//               them per row) 64 at a time, so the log-weights are read coalesced and each `loc` element serves kTile
//               trajectories from a register tile of kTile running sums;
//   pass 1    the scores' maxima (and whether a NaN was met) per trajectory — no exp;
//   pass 2    w = exp(s - smax), summed per chunk into LDS;
//   draw      per trajectory one wavefront adds the chunk sums up, finds the chunk in which u * total is crossed and
//             rescans that one chunk with a wavefront prefix scan: two passes plus a sliver of L / K of one.
//
// Every score is formed by the one function gaussian_scores (pairwise_gaussian.hpp: d ascending, ((t - l) * inv) squared
// into a fused multiply-add; `score_tile` is its N = kTile, the rescan's `score` its N = 1), so the particle that holds
// the maximum has w == 1 exactly in pass 2 and in the rescan.  The drawn particle always has positive weight: a crossing
// is only accepted on one, and a chunk whose sum says "crossed in here" while the rescan's own order of additions does
// not (a difference in the last place) yields its last particle of positive weight — which is also the clamp of the
// contract when u * total rounds to the total.
#include "ancestor_index.hpp"
#include "pairwise_gaussian.hpp"

namespace aesmc {

constexpr int kTile = 8;            // trajectories per workgroup: the register tile over m
constexpr int kBackThreads = 256;   // four wavefronts
constexpr int kBackWaves = kBackThreads / kWave;
constexpr int kBackMaxDim = 256;    // D the entry accepts: the target tile is kTile * D float64 of LDS
constexpr int kMaxChunks = 16;      // chunk sums per trajectory in LDS, whatever K is

template <typename T> struct BackwardArgs {
  const T *log_w;
  const T *loc, *target, *payload, *scale;
  int64_t loc_b, loc_k, loc_d, target_b, target_m, target_d, payload_b, payload_k, payload_p, scale_stride;
  const double *u;
  int64_t *idx;
  T *out_payload;
  int32_t *flags;
  int K, M, D, P, tiles, chunk, chunks;
};

// s[j] for the tile's kTile trajectories and particle k of batch row b
template <typename T>
__device__ __forceinline__ void score_tile(const BackwardArgs<T> &a, const double *tgt, const double *inv, int64_t b,
                                           int k, double (&s)[kTile]) {
  const double lw = (double)a.log_w[b * a.K + k];
  gaussian_scores<T, kTile>(a.loc + b * a.loc_b + (int64_t)k * a.loc_k, a.loc_d, tgt, kTile, inv, a.D, lw, s);
}

// the same for ONE trajectory of the tile (the rescan): the same function on column j of the tile, hence the same bits
template <typename T>
__device__ __forceinline__ double score(const BackwardArgs<T> &a, const double *tgt, const double *inv, int64_t b, int k,
                                        int j) {
  const double lw = (double)a.log_w[b * a.K + k];
  double s[1];
  gaussian_scores<T, 1>(a.loc + b * a.loc_b + (int64_t)k * a.loc_k, a.loc_d, tgt + j, kTile, inv, a.D, lw, s);
  return s[0];
}

template <typename T>
__global__ __launch_bounds__(kBackThreads) void backward_sample_kernel(const BackwardArgs<T> a) {
  __shared__ double tgt[kBackMaxDim * kTile];      // [d][j]
  __shared__ double inv[kBackMaxDim];
  __shared__ double wave_max[kBackWaves][kTile];
  __shared__ int wave_nan[kBackWaves];
  __shared__ double chunk_sum[kTile][kMaxChunks];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t b = blockIdx.x / a.tiles;
  const int m0 = (int)(blockIdx.x % a.tiles) * kTile;

  // the tile's targets (a trajectory beyond M repeats the last one and is never written) and 1 / scale
  stage_tile<T, kTile>(a.target + b * a.target_b, a.target_m, a.target_d, m0, a.M, a.scale, a.scale_stride, a.D, tid,
                       kBackThreads, tgt, inv);

  // ---- pass 1: maxima -------------------------------------------------------------------------------------------
  double smax[kTile];
  int nan_bits = 0;
#pragma unroll
  for (int j = 0; j < kTile; ++j) smax[j] = -__builtin_huge_val();
  for (int c = wave; c < a.chunks; c += kBackWaves) {
    const int k_end = min(a.K, (c + 1) * a.chunk);
    for (int k = c * a.chunk + lane; k < k_end; k += kWave) {
      double s[kTile];
      score_tile(a, tgt, inv, b, k, s);
#pragma unroll
      for (int j = 0; j < kTile; ++j) {
        nan_bits |= (s[j] != s[j]) ? (1 << j) : 0;
        smax[j] = fmax(smax[j], s[j]);      // (fmax drops a NaN operand: the bit above keeps it)
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    nan_bits |= __shfl_xor(nan_bits, off, kWave);
#pragma unroll
    for (int j = 0; j < kTile; ++j) smax[j] = fmax(smax[j], __shfl_xor(smax[j], off, kWave));
  }
  if (lane == 0) {
    wave_nan[wave] = nan_bits;
#pragma unroll
    for (int j = 0; j < kTile; ++j) wave_max[wave][j] = smax[j];
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBackWaves; ++w) {
    nan_bits |= wave_nan[w];
#pragma unroll
    for (int j = 0; j < kTile; ++j) smax[j] = fmax(smax[j], wave_max[w][j]);
  }

  // ---- pass 2: chunk sums of w = exp(s - smax) ---------------------------------------------------------------------
  // (a trajectory with a NaN or without a finite maximum: every difference is NaN or -inf, every w zero; unused)
  for (int c = wave; c < a.chunks; c += kBackWaves) {
    double sum[kTile];
#pragma unroll
    for (int j = 0; j < kTile; ++j) sum[j] = 0.0;
    const int k_end = min(a.K, (c + 1) * a.chunk);
    for (int k = c * a.chunk + lane; k < k_end; k += kWave) {
      double s[kTile];
      score_tile(a, tgt, inv, b, k, s);
#pragma unroll
      for (int j = 0; j < kTile; ++j) sum[j] += exp_nonpositive(s[j] - smax[j]);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int j = 0; j < kTile; ++j) sum[j] += __shfl_xor(sum[j], off, kWave);
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kTile; ++j) chunk_sum[j][c] = sum[j];
    }
  }
  __syncthreads();

  // ---- the draw: one wavefront per trajectory -----------------------------------------------------------------------
  for (int j = wave; j < kTile; j += kBackWaves) {
    const int m = m0 + j;
    if (m >= a.M) break;      // (wave-uniform, as everything below but the lanes' particles)
    double top = smax[0];
#pragma unroll
    for (int jj = 1; jj < kTile; ++jj) top = (jj == j) ? smax[jj] : top;
    const bool has_nan = (nan_bits >> j) & 1;
    int64_t drawn;
    if (has_nan || !(fabs(top) < __builtin_huge_val())) {
      if (lane == 0) raise_flag(a.flags, has_nan ? AESMC_FLAG_NAN_LOG_WEIGHT : AESMC_FLAG_DEGENERATE_ROW);
      drawn = a.K;
    } else {
      double total = 0.0;
      for (int c = 0; c < a.chunks; ++c) total += chunk_sum[j][c];
      double thr = a.u[b * a.M + m] * total;
      int pick = -1, last_positive = -1;
      double base = 0.0, run = 0.0;
      for (int c = 0; c < a.chunks; ++c) {
        const double cs = chunk_sum[j][c];
        const double next = run + cs;
        if (pick < 0 && next > thr) {
          pick = c;
          base = run;
        }
        if (cs > 0.0) last_positive = c;
        run = next;
      }
      if (pick < 0) {      // u * total rounded to the total: the clamp — the last particle of positive weight
        pick = last_positive;
        thr = __builtin_huge_val();
      }
      int found = -1, positive = -1;
      if (pick >= 0) {
        const int k_end = min(a.K, (pick + 1) * a.chunk);
        run = base;
        for (int k0 = pick * a.chunk; k0 < k_end && found < 0; k0 += kWave) {
          const int k = k0 + lane;
          double w = 0.0;
          if (k < k_end) w = exp_nonpositive(score(a, tgt, inv, b, k, j) - top);
          const double c = wave_inclusive_add(w, lane);
          const unsigned long long weighs = __ballot(w > 0.0);
          const unsigned long long crosses = __ballot(w > 0.0 && run + c > thr);
          if (weighs != 0) positive = k0 + 63 - __builtin_clzll(weighs);
          if (crosses != 0) found = k0 + __builtin_ctzll(crosses);
          run += __shfl(c, kWave - 1, kWave);
        }
      }
      // (the particle at the maximum has w == 1, so `positive` is set whenever `found` is not; K - 1 keeps the index in
      //  range whatever happens)
      drawn = found >= 0 ? found : (positive >= 0 ? positive : a.K - 1);
    }
    if (lane == 0) a.idx[b * a.M + m] = drawn;
    if (a.P > 0) {      // the tail: payload[b, idx] -> out_payload[b, m]; idx == K copies particle K - 1, as K3's clamp
      const int64_t source = drawn < a.K ? drawn : a.K - 1;
      const T *from = a.payload + b * a.payload_b + source * a.payload_k;
      T *to = a.out_payload + (b * a.M + m) * (int64_t)a.P;
      for (int p = lane; p < a.P; p += kWave) to[p] = from[(int64_t)p * a.payload_p];
    }
  }
}

template <typename T>
static int launch_backward_sample(const void *log_w, const aesmc_view3 *loc, const aesmc_view3 *target, const void *scale,
                                  int64_t scale_stride, const double *u, int64_t *out_idx, const aesmc_view3 *payload,
                                  void *out_payload, int32_t *flags, int64_t B, int64_t K, int64_t M, int64_t D, int64_t P,
                                  hipStream_t s) {
  BackwardArgs<T> a = {};
  a.log_w = (const T *)log_w;
  if (D > 0) {
    a.loc = (const T *)loc->ptr;
    a.loc_b = loc->stride_b, a.loc_k = loc->stride_k, a.loc_d = loc->stride_d;
    a.target = (const T *)target->ptr;
    a.target_b = target->stride_b, a.target_m = target->stride_k, a.target_d = target->stride_d;
    a.scale = (const T *)scale;
    a.scale_stride = scale_stride;
  }
  if (P > 0) {
    a.payload = (const T *)payload->ptr;
    a.payload_b = payload->stride_b, a.payload_k = payload->stride_k, a.payload_p = payload->stride_d;
    a.out_payload = (T *)out_payload;
  }
  a.u = u;
  a.idx = out_idx;
  a.flags = flags;
  a.K = (int)K, a.M = (int)M, a.D = (int)D, a.P = (int)P;
  a.tiles = (int)((M + kTile - 1) / kTile);
  // chunks: runs of a multiple of 64 particles, at most kMaxChunks of them
  a.chunk = kWave * (int)((K + (int64_t)kWave * kMaxChunks - 1) / ((int64_t)kWave * kMaxChunks));
  a.chunks = (int)((K + a.chunk - 1) / a.chunk);
  hipLaunchKernelGGL((backward_sample_kernel<T>), dim3((unsigned)(B * a.tiles)), dim3(kBackThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? AESMC_OK : AESMC_ERR_LAUNCH;
}

}  // namespace aesmc

extern "C" int aesmc_backward_sample(int dtype, const void *log_w, const aesmc_view3 *loc, const aesmc_view3 *target,
                                     const void *scale, int64_t scale_stride, const double *u, int64_t *out_idx,
                                     const aesmc_view3 *payload, void *out_payload, int32_t *flags, int64_t B, int64_t K,
                                     int64_t M, int64_t D, int64_t P, void *stream) {
  using namespace aesmc;
  if (log_w == nullptr || u == nullptr || out_idx == nullptr || B < 0 || K < 0 || M < 0 || D < 0 || P < 0 ||
      (((uintptr_t)u) & 7u) != 0 || (((uintptr_t)out_idx) & 7u) != 0)
    return AESMC_ERR_INVALID_ARGUMENT;
  if (dtype != AESMC_F32 && dtype != AESMC_F64) return AESMC_ERR_INVALID_ARGUMENT;
  if (D > 0 && (loc == nullptr || target == nullptr || scale == nullptr || loc->ptr == nullptr ||
                target->ptr == nullptr || (scale_stride != 0 && scale_stride != 1)))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (P > 0 && (payload == nullptr || payload->ptr == nullptr || out_payload == nullptr))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || M == 0) return AESMC_OK;
  if (K == 0) return AESMC_ERR_INVALID_ARGUMENT;      // trajectories to draw and no particle to draw them from
  if (D > kBackMaxDim) return AESMC_ERR_UNSUPPORTED;
  if (K > 0x3fffffffLL || M > 0x3fffffffLL || P > 0x7fffffffLL || B > 0x7fffffffLL ||
      B * ((M + kTile - 1) / kTile) > 0x7fffffffLL)
    return AESMC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AESMC_F32)
    return launch_backward_sample<float>(log_w, loc, target, scale, scale_stride, u, out_idx, payload, out_payload, flags,
                                         B, K, M, D, P, s);
  return launch_backward_sample<double>(log_w, loc, target, scale, scale_stride, u, out_idx, payload, out_payload, flags, B,
                                        K, M, D, P, s);
}
