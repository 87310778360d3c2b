// The expected complete-data sufficient statistics of a switching linear-Gaussian model from per-trajectory smoothed moments —
// aesmc_switching_moment_statistics (K45), aesmc_switching_masked_moment_statistics (K46) and
// aesmc_switching_statistics_finish of include/aesmc_hip.h: the E-step's reduction, from which an M-step or the score (Fisher's
// identity) is closed form on tiny matrices.
//
// A trajectory (b, n) has at time t the regime j = s_t, the smoothed N(m, P) of z_t, and (t >= 1) the regime i = s_{t-1}, the
// smoothed N(m', P') of z_{t-1} and cross[i,l] = Cov(z_{t,i}, z_{t-1,l}).  With x = (z, 1), X = D + 1, and o_c whether
// component c of y[b] was observed (K45: always), one launch adds to ROW j of a [16, F] array, per trajectory,
//
//   the emission block (every t)                                              columns
//     gram       E[x_t x_t^T], packed lower triangle, the one at index D        X (X + 1) / 2
//     obs_obs    o_c y_c^2                                                       Dy
//     obs_state  o_c y_c E[x_t]^T, [c][l]                                        Dy X
//     grams      (K46 only) o_c E[x_t x_t^T] for c = 0 .. Dy-1, packed           Dy X (X + 1) / 2
//   the transition block (t >= 1: regime_prev, mean_prev, cov_prev, cross given)
//     counts     1[s_{t-1} = i], i = 0 .. 15                                     16
//     next_next  E[z_t z_t^T], packed                                            D (D + 1) / 2
//     next_prev  E[z_t x_{t-1}^T] = [cross + m m'^T, m], [i][l]                   D X
//     prev_prev  E[x_{t-1} x_{t-1}^T], packed                                    X (X + 1) / 2
//
// in this order: F = aesmc_switching_statistics_columns(D, Dy, masked).  Packed: element (i, l), i >= l, at i (i + 1) / 2 + l.
// An entry such as P_il + m_i m_l is ONE float64 fused multiply-add; y_c^2 and y_c m_l are one rounded product.
//
// Geometry: 256 consecutive trajectories of the flattened [B N] range per tile, one lane per trajectory; a fixed grid of at
// most kStatGroups workgroups walks the tiles blockIdx.x, blockIdx.x + grid, ... (with few trajectories the 16-column tiles
// below are dealt out over gridDim.y workgroups each: see the launch).  A lane forms its payload 16 columns at a
// time (the operands of a column are read where it is formed: besides the two means and y no moment stays in a register),
// parks them in LDS as a float64 row of odd stride, and each wavefront contracts ITS 64 lanes on the float64 matrix cores:
// 16 steps of v_mfma_f64_16x16x4_f64 per 16 columns, A = the indicator regime[lane] == row, B = the parked columns (A of lane
// l: row l & 15 of trajectory 4 s + (l >> 4); B: column l & 15 of the same trajectory; result (row, column) = ((l >> 4) + 4
// reg, l & 15)).  The accumulator quads, one per 16 columns, live across the workgroup's tiles; at the end the four
// wavefronts' quads are added in wavefront order and stored over (accumulate = 0) or added to (1) the workgroup's slot of
// the workspace.  The kernel's columns are those of the padded extents (2, 4, 8 each; the emission block rounded up to a
// multiple of 16, so that the t = 0 form runs the emission block's MFMAs alone); the finishing launch adds the workgroups'
// slots in one fixed order (four interleaved slices of the workgroups, each ascending, then the slices in order) and
// writes the [16, F] array of the true extents.  No floating-point atomics, every sum has one order for given extents:
// the same operands give the same bits.
//
// 0 x NaN is NaN inside the matrix core, so what must not count is SELECTED to zero before it is parked: the lanes past the
// end of the range; the trajectory of a regime or previous regime outside [0, M), which also raises
// AESMC_FLAG_INDEX_OUT_OF_RANGE (K30's convention); in K46, y at an unobserved position, which is never read into a chain and
// may be NaN or Inf.  A NaN in a moment does poison its sums.
//
// Workspace (float64): [kStatGroups][column tiles][16 rows][16 columns].
//
// Compiler's resource report (-Rpass-analysis=kernel-resource-usage, gfx950, 256 lanes per workgroup):
//   <DP,DYP>  VGPRs  AGPRs  scratch B/lane  waves/SIMD       and of the masked instantiations (K46):
//   <2,2>       105     16        0             4              114     16        0             3
//   <2,4>       114     16        0             3              122     16        0             3
//   <2,8>       122     16        0             3              145     16        0             3
//   <4,2>       123     32        0             3              139     32        0             2
//   <4,4>       131     32        0             3              163     32        0             2
//   <4,8>       139     32        0             2              204     32        0             2
//   <8,2>       168     88        0             2              208     88        0             1
//   <8,4>       176     88        0             1              256     90        0             1
//   <8,8>       189     88        0             1              256    200        0             1
// The accumulator quads are the bulk of it (8 registers per 16 columns: 19 quads at <8,8>, 42 in its masked form) and the
// compiler hoists the loads of a tile's operands above its barrier; no instantiation uses scratch.
#include "switching_host.hpp"

namespace aesmc {

constexpr int kStatGroups = 512;            // workgroups of a launch at most: two per compute unit of an MI355X
constexpr int kStatTile = kSkBlock;         // trajectories per tile
constexpr int kStatStride = 17;             // float64 per parked row (16 columns, odd stride)
constexpr int kStatRows = kSkMaxRegimes;    // rows of the result: the matrix core's 16
typedef double stat_quad __attribute__((ext_vector_type(4)));

// ---- the column layout, of the true extents and of the padded ones alike --------------------------------------------------------
__host__ __device__ constexpr int stat_tri(int d) { return d * (d + 1) / 2; }
__host__ __device__ constexpr int stat_emission_columns(int d, int dy, bool masked) {
  return stat_tri(d + 1) + dy + dy * (d + 1) + (masked ? dy * stat_tri(d + 1) : 0);
}
__host__ __device__ constexpr int stat_transition_columns(int d) { return kStatRows + stat_tri(d) + d * (d + 1) + stat_tri(d + 1); }
__host__ __device__ constexpr int stat_columns(int d, int dy, bool masked) {
  return stat_emission_columns(d, dy, masked) + stat_transition_columns(d);
}
__host__ __device__ constexpr int stat_tiles16(int columns) { return (columns + 15) / 16; }
__host__ __device__ constexpr int stat_emission_tiles(int dp, int dyp, bool masked) {
  return stat_tiles16(stat_emission_columns(dp, dyp, masked));
}
__host__ __device__ constexpr int stat_all_tiles(int dp, int dyp, bool masked) {
  return stat_emission_tiles(dp, dyp, masked) + stat_tiles16(stat_transition_columns(dp));
}

// element e of a packed triangle over extent + 1 indices (the last one the constant's, where `with_one`) -> the same
// element's place in the triangle of the padded extent
__host__ __device__ inline int stat_pad_tri(int e, int d, int dp, bool with_one) {
  int i = 0;
  while (stat_tri(i + 1) <= e) ++i;
  int l = e - stat_tri(i);
  if (with_one && i == d) i = dp;
  if (with_one && l == d) l = dp;
  return stat_tri(i) + l;
}
// [r][l] of an [rows, d + 1] block -> the padded block's
__host__ __device__ inline int stat_pad_rect(int e, int d, int dp) {
  const int r = e / (d + 1), l = e - r * (d + 1);
  return r * (dp + 1) + (l == d ? dp : l);
}
// column c of the [16, F] result -> the kernel's column (of the padded extents, the transition block on a tile's boundary)
__host__ __device__ inline int stat_padded_column(int c, int d, int dy, int dp, int dyp, bool masked) {
  const int tx = stat_tri(d + 1), txp = stat_tri(dp + 1);
  int base = 0;
  if (c < tx) return stat_pad_tri(c, d, dp, true);
  c -= tx, base += txp;
  if (c < dy) return base + c;
  c -= dy, base += dyp;
  if (c < dy * (d + 1)) return base + stat_pad_rect(c, d, dp);
  c -= dy * (d + 1), base += dyp * (dp + 1);
  if (masked) {
    if (c < dy * tx) return base + (c / tx) * txp + stat_pad_tri(c % tx, d, dp, true);
    c -= dy * tx;
  }
  base = 16 * stat_emission_tiles(dp, dyp, masked);
  if (c < kStatRows) return base + c;
  c -= kStatRows, base += kStatRows;
  if (c < stat_tri(d)) return base + stat_pad_tri(c, d, dp, false);
  c -= stat_tri(d), base += stat_tri(dp);
  if (c < d * (d + 1)) return base + stat_pad_rect(c, d, dp);
  c -= d * (d + 1), base += dp * (dp + 1);
  return base + stat_pad_tri(c, d, dp, true);
}

struct StatArgs {
  const void *y;                       // [B,Dy]
  const uint8_t *observed;             // K46: [B,Dy], nonzero = observed; NULL in the unmasked instantiations
  const int32_t *regime, *regime_prev; // [B,N]; regime_prev NULL: the t = 0 form
  const double *mean_prev, *cov_prev, *cross, *mean, *cov;
  double *ws;
  int32_t *flags;
  int64_t total, tiles;                // B N, its tiles
  uint32_t N;
  int y_f32, M, D, Dy, accumulate;
};

// ---- the kernel's columns, known when it is compiled ----------------------------------------------------------------------------
enum StatKind { kStatZero, kStatGram, kStatObsObs, kStatObsState, kStatMaskedGram, kStatCount, kStatLagged, kStatGramPrev };
struct StatColumn {
  StatKind kind;
  int c, i, l;      // the observation's component; the element
};
constexpr StatColumn stat_tri_column(StatKind kind, int c, int e) {
  int i = 0;
  while (stat_tri(i + 1) <= e) ++i;
  return StatColumn{kind, c, i, e - stat_tri(i)};
}
// what column `at` of the padded layout holds; index DP of a gram is the constant's
constexpr StatColumn stat_column(int at, int dp, int dyp, bool masked) {
  const int tx = stat_tri(dp + 1), emission = 16 * stat_emission_tiles(dp, dyp, masked);
  if (at < emission) {
    if (at < tx) return stat_tri_column(kStatGram, 0, at);
    at -= tx;
    if (at < dyp) return StatColumn{kStatObsObs, at, 0, 0};
    at -= dyp;
    if (at < dyp * (dp + 1)) return StatColumn{kStatObsState, at / (dp + 1), 0, at % (dp + 1)};
    at -= dyp * (dp + 1);
    if (masked && at < dyp * tx) return stat_tri_column(kStatMaskedGram, at / tx, at % tx);
    return StatColumn{kStatZero, 0, 0, 0};
  }
  at -= emission;
  if (at < kStatRows) return StatColumn{kStatCount, 0, at, 0};
  at -= kStatRows;
  if (at < stat_tri(dp)) return stat_tri_column(kStatGram, 0, at);      // E[z_t z_t^T]: the gram's leading block
  at -= stat_tri(dp);
  if (at < dp * (dp + 1)) return StatColumn{kStatLagged, 0, at / (dp + 1), at % (dp + 1)};
  at -= dp * (dp + 1);
  if (at < tx) return stat_tri_column(kStatGramPrev, 0, at);
  return StatColumn{kStatZero, 0, 0, 0};
}

template <int... I, typename F> __device__ __forceinline__ void stat_each(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>)
template <int N, typename F> __device__ __forceinline__ void stat_for(F &&f) {
  stat_each(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f));
}

// What a lane keeps of its trajectory, and the columns it forms from it
template <int DP, int DYP, bool Masked> struct StatLane {
  double m[DP], mp[DP], y[DYP];        // zeros past the true extents; y zero where not observed
  bool seen[DYP];
  const double *cov, *cov_prev, *cross;
  int D, prev;                         // prev: s_{t-1}
  // E[x_i x_l] of x = (z, 1) ~ N(mu, P), i >= l, index DP the constant's
  template <int I, int L> __device__ __forceinline__ double second(const double *mu, const double *packed) const {
    if constexpr (I == DP) return L == DP ? 1.0 : mu[L < DP ? L : 0];
    else return __builtin_fma(mu[I], mu[L], I < D ? packed[sk_tri(I, L)] : 0.0);
  }
  template <int At> __device__ __forceinline__ double column() const {
    constexpr StatColumn col = stat_column(At, DP, DYP, Masked);
    if constexpr (col.kind == kStatGram) return second<col.i, col.l>(m, cov);
    else if constexpr (col.kind == kStatObsObs) return y[col.c] * y[col.c];
    else if constexpr (col.kind == kStatObsState) return col.l == DP ? y[col.c] : y[col.c] * m[col.l < DP ? col.l : 0];
    else if constexpr (col.kind == kStatMaskedGram) return seen[col.c] ? second<col.i, col.l>(m, cov) : 0.0;
    else if constexpr (col.kind == kStatCount) return prev == col.i ? 1.0 : 0.0;
    else if constexpr (col.kind == kStatLagged) {      // E[z_{t,i} x_{t-1,l}]
      if constexpr (col.l == DP) return m[col.i];
      else return __builtin_fma(m[col.i], mp[col.l], (col.i < D && col.l < D) ? cross[col.i * D + col.l] : 0.0);
    } else if constexpr (col.kind == kStatGramPrev) return second<col.i, col.l>(mp, cov_prev);
    else return 0.0;
  }
};

// LDS: [256][17] float64 parked columns (at the end: 4 x 256 of them the wavefronts' quads), [256] regimes
template <int DP, int DYP, bool Masked>
__global__ __launch_bounds__(kSkBlock) void switching_statistics_kernel(const StatArgs a) {
  constexpr int kEmissionTiles = stat_emission_tiles(DP, DYP, Masked), kTiles = stat_all_tiles(DP, DYP, Masked);
  __shared__ double park[kStatTile * kStatStride];
  __shared__ int seg[kStatTile];
  const int D = a.D, Dy = a.Dy, TD = D * (D + 1) / 2;
  const bool later = a.regime_prev != nullptr;      // (launch-uniform)
  const int p = threadIdx.x, wave = p / kWave, lane = p % kWave, ln = lane & 15, lgroup = lane >> 4;
  stat_quad acc[kTiles];
  stat_for<kTiles>([&](auto t) { acc[decltype(t)::value] = (stat_quad){0.0, 0.0, 0.0, 0.0}; });

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t n = tile * kStatTile + p;
    const bool live = n < a.total;
    const int64_t at = live ? n : a.total - 1;      // a lane past the end reads the last trajectory and counts for nothing
    const int s = a.regime[at], sp = later ? a.regime_prev[at] : 0;
    const bool inside = s >= 0 && s < a.M && sp >= 0 && sp < a.M;
    if (live && !inside) raise_flag(a.flags, AESMC_FLAG_INDEX_OUT_OF_RANGE);
    const bool valid = live && inside;
    seg[p] = valid ? s : -1;

    StatLane<DP, DYP, Masked> x;
    x.D = D, x.prev = sp;
    x.cov = a.cov + at * TD;
    x.cov_prev = later ? a.cov_prev + at * TD : x.cov;
    x.cross = later ? a.cross + at * D * D : x.cov;      // (not read in the t = 0 form)
    {
      const double *mrow = a.mean + at * D, *prow = later ? a.mean_prev + at * D : mrow;
#pragma unroll
      for (int i = 0; i < DP; ++i) x.m[i] = i < D ? mrow[i] : 0.0, x.mp[i] = (later && i < D) ? prow[i] : 0.0;
      const int64_t row = (at / a.N) * Dy;
#pragma unroll
      for (int c = 0; c < DYP; ++c) {
        const int64_t e = row + min(c, Dy - 1);
        bool seen = c < Dy;
        if constexpr (Masked) seen = seen && a.observed[e] != 0;
        const double v = a.y_f32 ? (double)static_cast<const float *>(a.y)[e] : static_cast<const double *>(a.y)[e];
        x.seen[c] = seen;
        x.y[c] = seen ? v : 0.0;
      }
    }
    __syncthreads();      // the regimes are parked
    int held[kWave / 4];      // regime of trajectory 4 s + (lane >> 4) of this wavefront, -1: contributes nothing
#pragma unroll
    for (int k = 0; k < kWave / 4; ++k) held[k] = seg[wave * kWave + 4 * k + lgroup];

    stat_for<kTiles>([&](auto tile16) {
      constexpr int t = decltype(tile16)::value;
      if (t >= kEmissionTiles && !later) return;      // (launch-uniform): the t = 0 form has no transition block
      if (t % gridDim.y != blockIdx.y) return;        // (workgroup-uniform): another workgroup's columns
      stat_for<16>([&](auto k) {
        park[p * kStatStride + decltype(k)::value] = valid ? x.template column<16 * t + decltype(k)::value>() : 0.0;
      });
      __syncthreads();
      stat_quad sum = acc[t];
#pragma unroll
      for (int s4 = 0; s4 < kWave / 4; ++s4) {
        const double left = held[s4] == ln ? 1.0 : 0.0;
        const double right = park[(wave * kWave + 4 * s4 + lgroup) * kStatStride + ln];
        sum = __builtin_amdgcn_mfma_f64_16x16x4f64(left, right, sum, 0, 0, 0);
      }
      acc[t] = sum;
      __syncthreads();      // the parked columns are read (after the last: the regimes too)
    });
  }

  // ---- the workgroup's partial: its four wavefronts' quads added in wavefront order ------------------------------------------------
  double *slot = a.ws + (int64_t)blockIdx.x * kTiles * 256;
  stat_for<kTiles>([&](auto tile16) {
    constexpr int t = decltype(tile16)::value;
    const bool formed = t < kEmissionTiles || later;      // (launch-uniform)
    if ((!formed && a.accumulate) || t % gridDim.y != blockIdx.y) return;
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) park[wave * 256 + (lgroup + 4 * reg) * 16 + ln] = acc[t][reg];
    __syncthreads();
    const double sum = formed ? ((park[p] + park[256 + p]) + park[512 + p]) + park[768 + p] : 0.0;
    slot[t * 256 + p] = a.accumulate ? slot[t * 256 + p] + sum : sum;
  });
}

// ---- the finishing launch ---------------------------------------------------------------------------------------------------------
// A block's 1024 threads are four slices of the workgroups times 256 elements of the [16, F] result: slice s adds the slots
// of workgroups s, s + 4, ... in ascending order, then the slices are added in order through LDS (K29 / K30's order)
constexpr int kStatFinishBlock = 1024, kStatFinishSlices = kStatFinishBlock / 256;

struct StatFinishArgs {
  const double *ws;
  double *out;      // [16, F]
  int D, Dy, dp, dyp, masked, columns, tiles, groups;
};

__global__ __launch_bounds__(kStatFinishBlock) void switching_statistics_finish_kernel(const StatFinishArgs a) {
  __shared__ double slices[kStatFinishBlock];
  const int t = threadIdx.x, e = t % 256, slice = t / 256;
  const int element = blockIdx.x * 256 + e;      // row * F + column
  const bool wanted = element < kStatRows * a.columns;
  double sum = 0.0;
  if (wanted) {
    const int row = element / a.columns, column = element - row * a.columns;
    const int from = stat_padded_column(column, a.D, a.Dy, a.dp, a.dyp, a.masked != 0);
    const double *cell = a.ws + (int64_t)(from >> 4) * 256 + row * 16 + (from & 15);
#pragma unroll 8
    for (int g = slice; g < a.groups; g += kStatFinishSlices) sum += cell[(int64_t)g * a.tiles * 256];
  }
  slices[t] = sum;
  __syncthreads();
  if (wanted && slice == 0) a.out[element] = ((slices[e] + slices[256 + e]) + slices[512 + e]) + slices[768 + e];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static inline int64_t stat_traj_tiles(int64_t B, int64_t N) { return (B * N + kStatTile - 1) / kStatTile; }
static inline int stat_groups(int64_t B, int64_t N) { return (int)std::min<int64_t>(stat_traj_tiles(B, N), kStatGroups); }
static inline bool stat_extents_ok(int64_t D, int64_t Dy) { return D >= 1 && Dy >= 1 && D <= kSkMaxDim && Dy <= kSkMaxDim; }

// K45, and K46 (`masked`: observed [B,Dy] given): one set of checks, one launch
static int stat_step(bool masked, int y_dtype, const void *y, const uint8_t *observed, const int32_t *regime,
                     const int32_t *regime_prev, const double *mean_prev, const double *cov_prev, const double *cross,
                     const double *mean, const double *cov, void *workspace, int accumulate, int32_t *flags, int64_t B,
                     int64_t N, int64_t M, int64_t D, int64_t Dy, void *stream) {
  if (masked && observed == nullptr) return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_observation(y, y_dtype) || regime == nullptr || mean == nullptr || cov == nullptr || workspace == nullptr ||
      B < 0 || N < 0 || !sk_extents_positive(M, D, Dy) || (accumulate != 0 && accumulate != 1))
    return AESMC_ERR_INVALID_ARGUMENT;
  const int given = (regime_prev != nullptr) + (mean_prev != nullptr) + (cov_prev != nullptr) + (cross != nullptr);
  if (given != 0 && given != 4) return AESMC_ERR_INVALID_ARGUMENT;      // (the operands of time t-1 come together)
  if (!sk_aligned(regime, 4) || !sk_aligned(regime_prev, 4) || !sk_aligned(mean_prev, 8) || !sk_aligned(cov_prev, 8) ||
      !sk_aligned(cross, 8) || !sk_aligned(mean, 8) || !sk_aligned(cov, 8) || !sk_aligned(workspace, 8) ||
      !sk_aligned(flags, 4))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (!sk_outputs_distinct({workspace}, {y, observed, regime, regime_prev, mean_prev, cov_prev, cross, mean, cov, flags}))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0) return AESMC_OK;
  if (!sk_extents_supported(M, D, Dy) || !sk_fits_32bit(B, N, kSkMaxDim * kSkMaxDim)) return AESMC_ERR_UNSUPPORTED;
  StatArgs a;
  a.y = y, a.observed = masked ? observed : nullptr;
  a.regime = regime, a.regime_prev = regime_prev;
  a.mean_prev = mean_prev, a.cov_prev = cov_prev, a.cross = cross, a.mean = mean, a.cov = cov;
  a.ws = static_cast<double *>(workspace);
  a.flags = flags;
  a.total = B * N, a.tiles = stat_traj_tiles(B, N), a.N = (uint32_t)N;
  a.y_f32 = y_dtype == AESMC_F32, a.M = (int)M, a.D = (int)D, a.Dy = (int)Dy, a.accumulate = accumulate;
  // Few trajectories: the 16-column tiles are dealt out over gridDim.y workgroups per group of trajectory tiles (tile t to
  // workgroup t mod gridDim.y), so that a launch fills the device and no workgroup walks every tile's load-and-barrier chain.
  // Every slot of the workspace still has one writer and every sum its one order: the bits do not depend on the split
  const int groups = stat_groups(B, N);
  return sk_for_extents(sk_pad(D), sk_pad(Dy), [&](auto d, auto dy) {
    return sk_for_flag(masked, [&](auto m) {
      constexpr int tiles = stat_all_tiles(decltype(d)::value, decltype(dy)::value, decltype(m)::value);
      return sk_launch(&switching_statistics_kernel<decltype(d)::value, decltype(dy)::value, decltype(m)::value>,
                       dim3((unsigned)groups, (unsigned)std::min(tiles, std::max(1, kStatGroups / 2 / groups))), dim3(kSkBlock),
                       0, (hipStream_t)stream, a);
    });
  });
}

}  // namespace aesmc

extern "C" int64_t aesmc_switching_statistics_columns(int64_t D, int64_t Dy, int masked) {
  using namespace aesmc;
  return stat_extents_ok(D, Dy) ? stat_columns((int)D, (int)Dy, masked != 0) : 0;
}

extern "C" int64_t aesmc_switching_statistics_workspace_bytes(int64_t D, int64_t Dy, int masked) {
  using namespace aesmc;
  if (!stat_extents_ok(D, Dy)) return 0;
  return (int64_t)kStatGroups * stat_all_tiles(sk_pad(D), sk_pad(Dy), masked != 0) * 256 * (int64_t)sizeof(double);
}

extern "C" int aesmc_switching_moment_statistics(int y_dtype, const void *y, const int32_t *regime,
                                                 const int32_t *regime_prev, const double *mean_prev,
                                                 const double *cov_prev, const double *cross, const double *mean,
                                                 const double *cov, void *workspace, int accumulate, int32_t *flags,
                                                 int64_t B, int64_t N, int64_t M, int64_t D, int64_t Dy, void *stream) {
  return aesmc::stat_step(false, y_dtype, y, nullptr, regime, regime_prev, mean_prev, cov_prev, cross, mean, cov, workspace,
                          accumulate, flags, B, N, M, D, Dy, stream);
}

extern "C" int aesmc_switching_masked_moment_statistics(int y_dtype, const void *y, const uint8_t *observed,
                                                        const int32_t *regime, const int32_t *regime_prev,
                                                        const double *mean_prev, const double *cov_prev,
                                                        const double *cross, const double *mean, const double *cov,
                                                        void *workspace, int accumulate, int32_t *flags, int64_t B,
                                                        int64_t N, int64_t M, int64_t D, int64_t Dy, void *stream) {
  return aesmc::stat_step(true, y_dtype, y, observed, regime, regime_prev, mean_prev, cov_prev, cross, mean, cov, workspace,
                          accumulate, flags, B, N, M, D, Dy, stream);
}

extern "C" int aesmc_switching_statistics_finish(const void *workspace, double *out, int masked, int64_t B, int64_t N,
                                                 int64_t D, int64_t Dy, void *stream) {
  using namespace aesmc;
  if (workspace == nullptr || out == nullptr || !sk_aligned(workspace, 8) || !sk_aligned(out, 8) ||
      (const void *)out == workspace || B < 0 || N < 0 || D < 1 || Dy < 1 || (masked != 0 && masked != 1))
    return AESMC_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0) return AESMC_OK;
  if (!stat_extents_ok(D, Dy) || !sk_fits_32bit(B, N, kSkMaxDim * kSkMaxDim)) return AESMC_ERR_UNSUPPORTED;
  StatFinishArgs f;
  f.ws = static_cast<const double *>(workspace), f.out = out;
  f.D = (int)D, f.Dy = (int)Dy, f.dp = sk_pad(D), f.dyp = sk_pad(Dy), f.masked = masked;
  f.columns = stat_columns(f.D, f.Dy, masked != 0);
  f.tiles = stat_all_tiles(f.dp, f.dyp, masked != 0), f.groups = stat_groups(B, N);
  const unsigned blocks = (unsigned)((kStatRows * f.columns + 255) / 256);
  return sk_launch(&switching_statistics_finish_kernel, dim3(blocks), dim3(kStatFinishBlock), 0, (hipStream_t)stream, f);
}
