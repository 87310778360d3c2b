/*
 * aesmc_hip.h — C ABI of libaesmc_hip.so, the MI355X (gfx950) kernels behind the batched SMC
 * inner loop of aesmc (reference: tuananhle7/aesmc, paths are into /root/reference).
 *
 * The reference has no FFI: its "operators" for this path are third-party CPU library calls made
 * from Python.  Each entry point below replaces one such call site; the Python host binds them
 * with ctypes (aesmc_amd/_lib.py) and INTEGRATION.md shows the stub a reference maintainer adds.
 *
 * Conventions (all entry points):
 *   - extern "C", return int status (AESMC_OK == 0), never throw, never allocate, never sync.
 *   - every pointer is a DEVICE pointer borrowed for the duration of the enqueued work;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - tensors are dense row-major [B, K, ...] unless a stride argument says otherwise;
 *   - `flags` is an optional device int32 word that kernels OR status bits into (AESMC_FLAG_*);
 *     the host reads it once per ELBO evaluation instead of synchronising per timestep.
 */
#ifndef AESMC_HIP_H_
#define AESMC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------------------------- */
#define AESMC_OK 0
#define AESMC_ERR_INVALID_ARGUMENT 1 /* null pointer, negative size, misaligned base pointer    */
#define AESMC_ERR_UNSUPPORTED 2      /* shape outside what the kernels handle (see each entry)  */
#define AESMC_ERR_LAUNCH 3           /* hipGetLastError() != hipSuccess after the launch        */
#define AESMC_ERR_WORKSPACE 4        /* workspace too small / missing                           */

/* ---- bits OR-ed into the device `flags` word ------------------------------------------------ */
#define AESMC_FLAG_NAN_LOG_WEIGHT 1  /* a log-weight was NaN  -> FloatingPointError, inference.py:244-245 */
#define AESMC_FLAG_DEGENERATE_ROW 2  /* a row had max = +-inf -> every index == K (reference: NaN CDF)     */
#define AESMC_FLAG_INDEX_OUT_OF_RANGE 4 /* gather saw idx < 0 or idx >= K (torch.gather would raise)     */
#define AESMC_FLAG_VALUE_OUTSIDE_SUPPORT 8 /* reserved for the host's deferred sample validation         */
#define AESMC_FLAG_UNSORTED_INDEX 16 /* gather backward was promised sorted indices and met a descent   */
#define AESMC_FLAG_INVALID_PARAMETER 32 /* reserved for the host's deferred distribution-argument validation */

/* ---- dtype tags ----------------------------------------------------------------------------- */
#define AESMC_F32 0
#define AESMC_F64 1

/* Library / build identification. */
/* 10000*major + 100*minor + patch.  History of the entry points (a binder checks this before it looks symbols up):
 *   100 (0.1.0)  rounds 1-2.
 *   200 (0.2.0)  removed aesmc_particle_mlp / aesmc_particle_mlp_max_hidden (the user's MLP stays in PyTorch);
 *                aesmc_set_step_parts / aesmc_set_sorted_backward_kernel became test hooks outside this header
 *                (aesmc_test_*); aesmc_affine_normal_propagate_drawn keeps its signature and now runs the fused launch
 *                (gather + noise + draw + log-weight terms in one kernel); added aesmc_affine_normal_propagate_wide
 *                (+ aesmc_affine_wide_dim, aesmc_affine_wide_workspace_bytes).
 *   500 (0.5.0)  aesmc_affine_normal_propagate_wide takes every width 17 .. 256 (observations 1 .. 256), dx != dy, any K
 *                (added aesmc_affine_wide_min_dim, aesmc_affine_wide_max_dim, aesmc_affine_wide_workspace_bytes_for);
 *                AESMC_FLAG_INVALID_PARAMETER reserved for the host's deferred distribution-argument validation;
 *                aesmc_particle_mlp is back (0.1.0 had it, 0.2.0 dropped it) WITH its backward: aesmc_particle_mlp_backward,
 *                aesmc_particle_mlp_backward_records (+ aesmc_particle_mlp_max_hidden); aesmc_particle_affine_tanh.
 *   501 (0.5.1)  added aesmc_affine_weight_pairs_scaled; aesmc_affine_weight_pairs_floats() grew by eight values (the
 *                three densities' constants and their tag behind the pairs: aesmc_affine_weight_pairs clears the tag);
 *                added aesmc_affine_normal_initial_step (K20: the first timestep's draw, emission location and
 *                log-weight in one launch).
 *                Additive since, version unchanged: aesmc_resample_step_stratified (K2's stratified sibling: one uniform
 *                per particle); aesmc_backward_sample (K21: one step of backward simulation, FFBS);
 *                aesmc_pairwise_lse (K22: the pairwise log-sum-exp of the marginal smoother, FFBSm);
 *                aesmc_pairwise_mean (K23: the pairwise softmax mean of the two-slice smoother);
 *                aesmc_pairwise_argmax (K24: the pairwise max and argmax of the MAP trajectory, particle Viterbi);
 *                aesmc_pairwise_pass (K25: the backward of K22, for the marginal particle filter's objective);
 *                aesmc_resample_step_packed, aesmc_affine_normal_propagate_drawn_packed,
 *                aesmc_affine_step_backward_packed, aesmc_unpack_ancestors (a step's ancestry handed from K2 to K16 /
 *                K14 as one 32-bit word per particle);
 *                aesmc_conditional_ancestor_index (K26: conditional multinomial resampling with ancestor sampling,
 *                the resampling step of particle Gibbs);
 *                aesmc_affine_quadratic_logweight, aesmc_adapted_draw (K27, K28: the first-stage weights and the draw of
 *                a fully adapted auxiliary particle filter step);
 *                aesmc_affine_quadratic_logweight_backward, aesmc_adapted_draw_backward,
 *                aesmc_adapted_backward_workspace_bytes (K29, K30: their adjoints, for training through the adapted filter);
 *                aesmc_switching_kalman_step with aesmc_switching_max_latent_dim, aesmc_switching_max_observation_dim,
 *                aesmc_switching_max_regimes (K31: one step of the Rao-Blackwellised filter of a switching
 *                linear-Gaussian model);
 *                aesmc_switching_lookahead, aesmc_switching_kalman_draw (K32, K33: the exact first-stage weights and regime
 *                posteriors of that model, and K31's step with the regime drawn from them — its fully adapted filter);
 *                aesmc_switching_information_step, aesmc_switching_backward_scores (K34, K35: Rao-Blackwellised backward
 *                simulation over the stored systems of either filter — its smoother);
 *                aesmc_switching_smooth_combine (K36: the smoothed moments and lag-one cross-covariance of the continuous
 *                state along a regime trajectory, from the conditional filter and K34 — the two-filter state smoother);
 *                aesmc_switching_conditional_ancestor_index with aesmc_switching_conditional_max_particles,
 *                aesmc_switching_kalman_conditional_step (K37, K38: conditional resampling with ancestor sampling against
 *                K34's information, and K31's step with one slot's regime pinned — particle Gibbs on the regimes);
 *                aesmc_switching_kalman_masked_step, aesmc_switching_masked_lookahead,
 *                aesmc_switching_masked_information_step, aesmc_switching_masked_smooth_combine (K39, K40, K41, K42: K31 /
 *                K33 / K38, K32, K34 and K36 with a per-row mask of the observation's components — missing observations,
 *                and forecasts as steps with nothing observed);
 *                aesmc_switching_lookahead_scores, aesmc_switching_masked_lookahead_scores,
 *                aesmc_switching_optimal_resample with aesmc_switching_optimal_resample_max_candidates (K43, K44: the
 *                look-ahead's scores and optimal resampling over all successor regimes — the discrete particle filter);
 *                aesmc_switching_moment_statistics, aesmc_switching_masked_moment_statistics,
 *                aesmc_switching_statistics_finish with aesmc_switching_statistics_columns and
 *                aesmc_switching_statistics_workspace_bytes (K45, K46: the expected sufficient statistics of that model from
 *                per-trajectory smoothed moments — the E-step's reduction, for EM and the score);
 *                aesmc_switching_state_draw (K47: a draw of the continuous state path given a regime path, the whole
 *                backward pass of forward filtering, backward sampling in one launch — for Gibbs on all parameters);
 *                aesmc_switching_lookahead_conditional_ancestor_index, its masked form
 *                aesmc_switching_masked_lookahead_conditional_ancestor_index, with
 *                aesmc_switching_lookahead_conditional_max_particles, and aesmc_switching_kalman_conditional_draw (K48, K49:
 *                the look-ahead and the conditional ancestors in one launch, and K31's step with the regime drawn from the
 *                ancestor's posterior row and one slot pinned — look-ahead particle Gibbs on the regimes);
 *                aesmc_switching_collapse, aesmc_switching_pair_smooth (K50, K51: the moment-matching collapse of Gaussian
 *                mixtures and a Rauch-Tung-Striebel step between mixture components — the deterministic collapsed-mixture
 *                filter and smoother, GPB2 / Kim's filter and IMM);
 *                aesmc_switching_kalman_step_backward, aesmc_switching_kalman_masked_step_backward,
 *                aesmc_switching_backward_workspace_bytes, aesmc_switching_collapse_backward (K52, K53, K54: the adjoints
 *                of K31 / K39 with the regime given and of K50 — the gradient of the collapsed-mixture evidence).
 *   400 (0.4.0)  aesmc_affine_chain grew `pairs_in` / `pairs_out` (a run of backward steps builds the weight pairs once);
 *                added aesmc_wide_adjoint_tile, aesmc_wide_adjoint_scale, aesmc_wide_adjoint_merge
 *   300 (0.3.0)  added aesmc_affine_normal_propagate_drawn_paired, aesmc_affine_weight_pairs,
 *                aesmc_affine_weight_pairs_floats (round 5: packed multiply-adds in the fused propagation launch). */
int aesmc_version(void);
const char *aesmc_target_arch(void); /* "gfx950" */

/* The address kernels can use for a pointer into PINNED host memory (hipHostMalloc / PyTorch pin_memory=True), or
 * AESMC_ERR_UNSUPPORTED when it is not mapped into the device's address space.  aesmc/inference.py:250 draws one
 * uniform per batch row on the host before every resampling step: with this, `u` of aesmc_ancestor_index /
 * aesmc_resample_step may point at the pinned block the host wrote them into — 8 bytes per row read over the host
 * link — instead of at a device copy made by a launch of its own per timestep. */
int aesmc_host_device_pointer(const void *host_ptr, void **device_ptr);

/*
 * K1 — fused log-weight combine + per-row log-sum-exp.
 *   lw[b,k]  = lp_a[b,k] + lp_b[b,k] - lp_c[b,k]           (lp_b / lp_c may be NULL: term dropped)
 *   lse[b]   = log sum_k exp(lw[b,k])                      (out_lse may be NULL)
 * Replaces: the two elementwise torch ops at aesmc/inference.py:97-98 and :125-126, and the
 * torch.logsumexp of aesmc/inference.py:130 / :158 and aesmc/math.py:28 (per timestep, no stack).
 * out_lw may be NULL (pure row-LSE of lp_a).  out_lw may alias lp_a.  Inputs dense [B,K].
 * Special values follow torch.logsumexp: row of -inf -> -inf; any +inf -> +inf; any NaN -> NaN.
 */
int aesmc_logweight_lse(int dtype, const void *lp_a, const void *lp_b, const void *lp_c,
                        void *out_lw, void *out_lse, int64_t B, int64_t K, void *stream);

/*
 * K1 with a running sum over time — importance sampling with more than one timestep normalises the
 * SUM of the per-step log-weights (aesmc/inference.py:156-159: torch.sum of a stack of all T weight
 * tensors, then torch.logsumexp).  One launch per step instead:
 *   lw[b,k]      = lp_a + lp_b - lp_c          (as K1; out_lw may be NULL when the step's own
 *                                               weights are not wanted)
 *   out_acc[b,k] = acc_in[b,k] + lw[b,k]       (left to right over time: the order torch.sum takes
 *                                               over the leading dim of the stack)
 *   out_lse[b]   = log sum_k exp(out_acc[b,k]) (may be NULL; asked for at the last step only)
 * out_acc may alias acc_in.  Same special values as K1.
 */
int aesmc_logweight_accumulate(int dtype, const void *lp_a, const void *lp_b, const void *lp_c,
                               const void *acc_in, void *out_lw, void *out_acc, void *out_lse,
                               int64_t B, int64_t K, void *stream);

/*
 * K1 backward.  g[b,k] = grad_lw[b,k] + grad_lse[b] * exp(lw[b,k] - lse[b])   (either grad may be
 * NULL = zero).  Writes out_g (gradient w.r.t. lp_a and lp_b) and, if non-NULL, out_neg_g = -g
 * (gradient w.r.t. lp_c).  Replaces autograd of the ops listed under K1.
 * Where lse[b] is not finite the kernel evaluates the expression as written: lse = -inf (a row of -inf) gives
 * exp(-inf + inf) = NaN times grad_lse, lse = +inf gives exp(-inf) = 0 for finite lw and NaN where lw = +inf, a NaN lse
 * gives NaN; with grad_lse NULL the term is dropped and g = grad_lw whatever lse holds.
 * (Test hooks outside this header, like the other aesmc_test_*: aesmc_test_last_logweight_form reports the form the
 * last K1 launch took, forward or backward, as 2 * TPR + VEC; aesmc_test_last_particle_summary_form does so for K7.)
 */
int aesmc_logweight_lse_backward(int dtype, const void *lw, const void *lse, const void *grad_lw,
                                 const void *grad_lse, void *out_g, void *out_neg_g, int64_t B,
                                 int64_t K, void *stream);

/*
 * K2 — systematic ancestral resampling, one independent problem per batch row.
 *   w        = exp(log_w[b,:] - max_k log_w[b,:])                 (evaluated in float64)
 *   c[j]     = (w[0] + ... + w[j]) / (w[0] + ... + w[K-1])        (float64 segmented prefix scan)
 *   pos[k]   = (u[b] + k) / K                                     (float64, true division)
 *   idx[b,k] = #{ j : c[j] <= pos[k] }                            (== np.digitize(pos, c))
 * Replaces aesmc/inference.py:234-269 (numpy uniform draw excluded: `u` [B] float64 comes from the
 * host's numpy global RandomState so RNG consumption is unchanged) and aesmc/math.py:33-51 on the
 * numpy branch.  NaN anywhere -> AESMC_FLAG_NAN_LOG_WEIGHT (reference raises FloatingPointError);
 * rows whose max is +-inf -> every idx == K and AESMC_FLAG_DEGENERATE_ROW (reference: NaN CDF makes
 * np.digitize return K).  `ws` is needed only when K > aesmc_ancestor_index_lds_max_particles():
 * then it must hold aesmc_workspace_bytes(B, K) bytes.
 */
int aesmc_ancestor_index(int dtype, const void *log_w, const double *u, int64_t *out_idx,
                         int32_t *flags, int64_t B, int64_t K, void *ws, size_t ws_bytes,
                         void *stream);
int64_t aesmc_ancestor_index_lds_max_particles(void);
size_t aesmc_workspace_bytes(int64_t B, int64_t K);

/*
 * K3 — resample gather:  dst[b,k,:] = src[b, idx[b,k], :]  with `row_bytes` contiguous bytes per
 * particle.  src may be strided in its first two dims (byte strides src_stride_b / src_stride_k;
 * this covers the transposed time-0 latent of aesmc/state.py:102-103); dst is dense.
 * Replaces torch.gather at aesmc/state.py:179 (and aesmc/inference.py:226 with row_bytes = 8).
 * idx outside [0,K) never faults: it is clamped and AESMC_FLAG_INDEX_OUT_OF_RANGE is raised.
 */
int aesmc_resample_gather(const void *src, const int64_t *idx, void *dst, int32_t *flags,
                          int64_t B, int64_t K, int64_t row_bytes, int64_t src_stride_b,
                          int64_t src_stride_k, void *stream);

/*
 * K3 backward:  grad_src[b,j,:] = sum_{k : idx[b,k]==j} grad_out[b,k,:]   (`row_elems` elements of
 * `dtype` per particle, both tensors dense).  grad_src is fully overwritten (zero where a particle
 * has no offspring).  Replaces the scatter_add autograd of torch.gather (aesmc/state.py:179).
 * index_is_sorted != 0 promises idx non-decreasing along k (true for every output of
 * aesmc_ancestor_index): the segmented-sum kernel without atomics is used and a violation raises
 * AESMC_FLAG_UNSORTED_INDEX; 0 selects the order-agnostic kernel (one float atomic per run).
 */
int aesmc_resample_gather_backward(int dtype, const void *grad_out, const int64_t *idx,
                                   void *grad_src, int32_t *flags, int64_t B, int64_t K,
                                   int64_t row_elems, int index_is_sorted, void *stream);

/*
 * K4 — summed Normal log-density:
 *   out[b,k] = sum_{j<D} ( -((v-mu)^2) / (2 sigma^2) - log(sigma) - log(sqrt(2 pi)) )
 * with v = value[b,k,j], mu = loc[b,k,j], sigma = scale[b,k,j]; each operand is a [B,K,D] VIEW given
 * by its element strides (sb, sk, sd), 0 meaning broadcast along that dim.  out is dense [B,K].
 * Replaces, inside aesmc/state.py:114-155 (`state.log_prob`), torch.distributions.Normal.log_prob
 * followed by `.view(B, K, -1).sum(2)` (state.py:143-151) — about eleven launches per call —
 * element arithmetic in PyTorch's own order.
 */
int aesmc_normal_logprob_sum(int dtype, const void *value, const void *loc, const void *scale,
                             void *out, int64_t B, int64_t K, int64_t D, int64_t value_sb,
                             int64_t value_sk, int64_t value_sd, int64_t loc_sb, int64_t loc_sk,
                             int64_t loc_sd, int64_t scale_sb, int64_t scale_sk, int64_t scale_sd,
                             void *stream);

/*
 * K4 backward.  grad_out dense [B,K]; each non-NULL grad_* is written densely [B,K,D]:
 *   grad_value = -g z,  grad_loc = g z,  grad_scale = g ((v-mu)^2 / sigma^3 - 1/sigma),
 *   z = (v-mu)/sigma^2.  Reduction over broadcast dims is left to the caller (autograd's expand).
 */
int aesmc_normal_logprob_sum_backward(int dtype, const void *value, const void *loc,
                                      const void *scale, const void *grad_out, void *grad_value,
                                      void *grad_loc, void *grad_scale, int64_t B, int64_t K,
                                      int64_t D, int64_t value_sb, int64_t value_sk, int64_t value_sd,
                                      int64_t loc_sb, int64_t loc_sk, int64_t loc_sd,
                                      int64_t scale_sb, int64_t scale_sk, int64_t scale_sd,
                                      void *stream);

/*
 * K5 — the whole log-weight of one SMC step when the prior / transition, the emission and the
 * proposal are all Normal:
 *   lw[b,k] = sum_j log N(x; mu_p, s_p) + sum_j log N(y; mu_g, s_g) - sum_j log N(x; mu_q, s_q)
 * `views` points to eight [B,K,D] views (element strides, 0 = broadcast) in this order:
 *   0 x (latent, extent Dx)   1 mu_p   2 s_p      (prior or transition)
 *   3 y (observation, Dy)     4 mu_g   5 s_g      (emission)
 *   6 mu_q (extent Dx)        7 s_q               (proposal, evaluated at x)
 * Replaces three calls of K4 and the combine of K1 (aesmc/inference.py:112-126 via
 * aesmc/state.py:114-155); bit-identical to that route.
 * Covered operands:
 *   - extents Dx, Dy <= 64: any scales — one value for the whole tensor (all strides 0, e.g.
 *     Normal(loc, 0.7): the fastest kernels), a per-dimension vector, or a full [B,K,D] view;
 *   - extents above 64: scalar scales only, and only when Dx and Dy take the same lane team in K4,
 *     each row is a multiple of 16 bytes, contiguous and 16-byte aligned.
 * Anything else returns AESMC_ERR_UNSUPPORTED and the caller takes the K4 + K1 route (same numbers).
 */
typedef struct aesmc_view3 {
  const void *ptr;
  int64_t stride_b, stride_k, stride_d; /* element strides, 0 = broadcast */
} aesmc_view3;

int aesmc_normal_logweight(int dtype, const aesmc_view3 *views, void *out_lw, int64_t B, int64_t K,
                           int64_t Dx, int64_t Dy, void *stream);

/* K5 backward: gradients of aesmc_normal_logweight with respect to the values, the locations and
 * the scales, each written densely over [B,K,Dx] (grad_x, grad_mu_p, grad_mu_q, grad_s_p, grad_s_q)
 * or [B,K,Dy] (grad_y, grad_mu_g, grad_s_g); NULL outputs are skipped; a broadcast operand's
 * gradient is reduced by the caller (autograd's expand-backward).  `views` as for the forward (any
 * scales), grad_lw [B,K].  Bit-identical to three aesmc_normal_logprob_sum_backward launches (with
 * -grad_lw for the proposal term) and the add grad_x = grad_x_p + grad_x_q.
 */
int aesmc_normal_logweight_backward(int dtype, const aesmc_view3 *views, const void *grad_lw, void *grad_x,
                                    void *grad_mu_p, void *grad_y, void *grad_mu_g, void *grad_mu_q,
                                    void *grad_s_p, void *grad_s_g, void *grad_s_q, int64_t B, int64_t K,
                                    int64_t Dx, int64_t Dy, void *stream);

/* K5 backward fused with K1's: the gradient of  lse[b] = logsumexp_k lw[b,k]  (and, optionally, of lw
 * itself) with respect to K5's operands in one launch —
 *   g[b,k] = grad_lse[b] * exp(lw[b,k] - lse[b])  (+ grad_lw[b,k] when grad_lw is not NULL)
 * is formed per element where aesmc_normal_logweight_backward would read grad_lw, with K1's own
 * operations, so the results equal aesmc_logweight_lse_backward followed by
 * aesmc_normal_logweight_backward bit for bit, without the [B,K] round trip and the launch.
 * `lw` is what aesmc_normal_logweight produced for `views`; lse, grad_lse are [B].  Replaces the
 * autograd chain of aesmc/inference.py:112-132 for one timestep. */
int aesmc_normal_logweight_lse_backward(int dtype, const aesmc_view3 *views, const void *lw, const void *lse,
                                        const void *grad_lse, const void *grad_lw, void *grad_x,
                                        void *grad_mu_p, void *grad_y, void *grad_mu_g, void *grad_mu_q,
                                        void *grad_s_p, void *grad_s_g, void *grad_s_q, int64_t B, int64_t K,
                                        int64_t Dx, int64_t Dy, void *stream);

/* Fused resampling step — K2, plus two optional by-products of having the whole batch row in one
 * workgroup:
 *   out_lse[b] = logsumexp_k log_w[b,k]  (dtype of log_w; the row's term of log Z,
 *                aesmc/inference.py:130-132), computed in float64 from K2's own max and sum — the
 *                special rows give what K1 gives (NaN, +inf, -inf);
 *   dst[b,k,:] = src[b, out_idx[b,k], :]  (K3's contract for ONE payload tensor,
 *                aesmc/state.py:158-183), with the indices taken from LDS instead of HBM.
 * `out_lse` may be NULL; `src` and `dst` are NULL together.  out_idx is always written and equals
 * aesmc_ancestor_index's bit for bit; dst equals aesmc_resample_gather's (rows of a degenerate
 * batch row: source row K-1, as K3's clamp gives).  Returns AESMC_ERR_UNSUPPORTED — caller takes
 * K2 then K3 — when K exceeds aesmc_ancestor_index_lds_max_particles(), or the payload rows are
 * not multiples of 4 bytes / dst is not 16-byte aligned with a 16-byte batch-row pitch.
 */
int aesmc_resample_step(int dtype, const void *log_w, const double *u, int64_t *out_idx, void *out_lse,
                        const void *src, void *dst, int32_t *flags, int64_t B, int64_t K,
                        int64_t row_bytes, int64_t src_stride_b, int64_t src_stride_k, void *stream);

/* K2 with the children ranges as a by-product: aesmc_resample_step without a payload, plus
 *   out_child_end[b,k] = #{k' : out_idx[b,k'] <= k}      (int32 [B,K])
 * — the ancestor indices are non-decreasing along k, so the children of particle k are the positions
 * [out_child_end[b,k-1], out_child_end[b,k]) (0 for k = 0): what torch.gather's backward (aesmc/state.py:179) sums
 * per particle, handed to aesmc_affine_step_backward_resampled so that it forms those sums where it consumes them.
 * The scan has the value in a register anyway: 4 more bytes per particle written. */
int aesmc_resample_step_ranges(int dtype, const void *log_w, const double *u, int64_t *out_idx, void *out_lse,
                               int32_t *out_child_end, int32_t *flags, int64_t B, int64_t K, void *stream);

/* K2 handing its results to the launches of this library that consume them as ONE 32-bit word per particle:
 *   out_words[b,k] = out_idx[b,k] | out_child_end[b,k] << 16      (uint32 [B,K], 16-byte aligned)
 * — aesmc_resample_step_ranges' two arrays (12 bytes per particle) in 4: the index (K for a NaN / degenerate row, flagged
 * as there) and the children's range (0 .. K) both fit 16 bits.  `want_child_end` == 0 leaves the high halves 0
 * (aesmc_resample_step without a payload).  out_lse, flags: as aesmc_resample_step.  The words are read by
 * aesmc_affine_normal_propagate_drawn_packed (low halves) and aesmc_affine_step_backward_packed; aesmc_unpack_ancestors
 * turns them back into the two arrays for everything else.  AESMC_ERR_UNSUPPORTED (nothing launched; take
 * aesmc_resample_step[_ranges]) unless a row is whole wavefronts of the kernel's particles per lane — K a multiple of 256
 * from 768 to 4096, of 512 up to 8192, of 1024 up to 16384, of 2048 up to 32768, and log_w 16-byte aligned —: exactly the
 * rows for which aesmc_resample_step[_ranges] without a payload runs the same kernel body, so the two give the same bits
 * (rows of at most 512 particles run another kernel there, and are declined here). */
int aesmc_resample_step_packed(int dtype, const void *log_w, const double *u, uint32_t *out_words, void *out_lse,
                               int want_child_end, int32_t *flags, int64_t B, int64_t K, void *stream);

/* out_idx[b,k] = words[b,k] & 0xffff (int64), out_child_end[b,k] = words[b,k] >> 16 (int32; NULL: not wanted): the packed
 * words of aesmc_resample_step_packed as the arrays of aesmc_resample_step_ranges.  K <= 65535. */
int aesmc_unpack_ancestors(const uint32_t *words, int64_t *out_idx, int32_t *out_child_end, int64_t B, int64_t K,
                           void *stream);

/* K2's stratified sibling — one independent uniform per particle instead of one per batch row:
 *   c[j]     as K2's                                             (float64; the same arithmetic, operation for operation)
 *   pos[k]   = min((u[b,k] + k) / K, 1 - 2^-53)                  (float64: sum, true division, clamp; `u` is [B,K])
 *   idx[b,k] = #{ j : c[j] <= pos[k] }
 * Exactly one position per stratum [k/K, (k+1)/K], so the indices are non-decreasing along k like K2's and everything
 * that consumes them (aesmc_resample_gather_backward's sorted form, aesmc_affine_step_backward_resampled, the fused
 * propagation launches) takes them unchanged.  The clamp keeps a position that u + (K-1) rounded up to 1.0 inside the
 * last stratum: a row with a finite maximum never yields the index K.  NaN rows and rows whose maximum is +-inf: K2's
 * conventions (idx == K, the flag bits, out_lse as aesmc_resample_step's).
 * By-products as aesmc_resample_step / aesmc_resample_step_ranges define them, each may be NULL:
 *   out_lse[b]         = logsumexp_k log_w[b,k]                  (dtype of log_w)
 *   out_child_end[b,k] = #{k' : out_idx[b,k'] <= k}              (int32 [B,K]; monotone on knife-edge rows too)
 * There is no payload tail: a caller that reads resampled values gathers with aesmc_resample_gather.
 * K up to aesmc_ancestor_index_lds_max_particles() is resolved inside one workgroup; a larger K goes through `ws`
 * (aesmc_workspace_bytes(B, K) bytes, else AESMC_ERR_WORKSPACE) and delivers the indices only: asked for a by-product
 * there the entry returns AESMC_ERR_UNSUPPORTED and launches nothing (the caller composes K1 / the ranges itself).
 */
int aesmc_resample_step_stratified(int dtype, const void *log_w, const double *u, int64_t *out_idx, void *out_lse,
                                   int32_t *out_child_end, int32_t *flags, int64_t B, int64_t K, void *ws,
                                   size_t ws_bytes, void *stream);

/* K21 — one backward step of forward filtering / backward simulation (FFBS; Godsill, Doucet & West 2004): M
 * trajectories per batch row each draw one of the filter's K stored particles of step t, in proportion to its weight
 * times the transition density from it to the trajectory's state at t+1.  The reference has no such call site: its one
 * smoothed posterior is the genealogy (aesmc/inference.py:196-231), which collapses over long sequences.
 *   log_w   T [B,K] dense                 the filter's step-t log-weights
 *   loc     T [B,K,D] view                the transition's location for every stored particle
 *   target  T [B,M,D] view                the trajectories' states at t+1 (`stride_k` steps along m)
 *   scale   T, D values                   read with the element stride `scale_stride`: 0 (one value) or 1
 *   u       float64 [B,M] dense           in [0, 1)
 * T is float32 or float64 (`dtype`); D == 0 (loc / target / scale may be NULL) means no transition term: the draw at the
 * last timestep.  All arithmetic is in float64 whatever T is:
 *   inv[d]   = 1 / (double)scale[d]
 *   q[m,k]   = sum_d ((double)target[b,m,d] - (double)loc[b,k,d])^2 * inv[d]^2   (as ((t - l) * inv)^2, d ascending)
 *   s[m,k]   = (double)log_w[b,k] - 0.5 * q[m,k]
 *   smax[m]  = max_k s[m,k]
 *   w[m,k]   = exp(s[m,k] - smax[m])                                            (K2's float64 exp of a non-positive number)
 *   C[m,k]   = w[m,0] + ... + w[m,k]
 *   idx[b,m] = min( #{k : C[m,k] <= u[b,m] * C[m,K-1]},  max{k : w[m,k] > 0} )
 * The Normal's normalising constant is the same for every k (the scale does not depend on the particle) and is dropped.
 * The order of the two sums (over d, over k) and the contraction of multiply-adds are the kernel's: a difference in the
 * last place decides an index only on a knife edge of measure zero (K2's stance).  The `min` is the clamp: u * C[K-1] can
 * round to C[K-1] itself, the count is then K and the last particle of positive weight is the answer; the drawn particle
 * always has positive weight.
 * Bad rows, per (b, m), by K2's conventions: any NaN among s[m,:] raises AESMC_FLAG_NAN_LOG_WEIGHT and idx = K; an smax
 * that is not finite (all -inf, or a +inf) raises AESMC_FLAG_DEGENERATE_ROW and idx = K.
 * Optional tail (P > 0): out_payload[b,m,:] = payload[b, idx[b,m], :] with `payload` a T [B,K,P] view and out_payload
 * dense [B,M,P] (K3 cannot serve: its index tensor has the payload's own particle count); idx == K copies particle K-1,
 * clamped as in K3, and nothing is ever read out of bounds.
 * No workspace, K not bounded by LDS.  D above 256 returns AESMC_ERR_UNSUPPORTED and launches nothing; B M == 0 is a
 * no-op; K == 0 with trajectories to draw is AESMC_ERR_INVALID_ARGUMENT.
 */
int aesmc_backward_sample(int dtype, const void *log_w, const aesmc_view3 *loc, const aesmc_view3 *target,
                          const void *scale, int64_t scale_stride, const double *u, int64_t *out_idx,
                          const aesmc_view3 *payload, void *out_payload, int32_t *flags, int64_t B, int64_t K, int64_t M,
                          int64_t D, int64_t P, void *stream);

/* K22 — a pairwise Gaussian log-sum-exp: the building block of the marginal particle smoother (FFBSm; Huerzeler &
 * Kuensch 1998; Doucet, Godsill & Andrieu 2000), which re-weights the particles the filter stored instead of drawing
 * trajectories from them (K21).  The reference has no such call site.  For every batch row b and row point r:
 *   out[b,r] = row_add[b,r] + log sum_c exp( term[b,c] - 1/2 sum_d ((rows[b,r,d] - cols[b,c,d]) / scale[d])^2 )
 *   rows     T [B,R,D] view               the row points (`stride_k` steps along r)
 *   cols     T [B,C,D] view               the columns (`stride_k` steps along c)
 *   scale    T, D values                  read with the element stride `scale_stride`: 0 (one value) or 1
 *   col_a    T [B,C] dense                a log-weight per column; -inf: the column is absent
 *   col_sub  T [B,C] dense or NULL        subtracted from col_a (NULL: 0)
 *   row_add  T [B,R] dense or NULL        added to the result (NULL: 0)
 *   out      T [B,R] dense
 * One backward step of FFBSm is two launches: the denominators den[b,j] (rows = the particles of step t+1, cols = the
 * transition's locations of step t's particles, col_a = log_w_t), then the smoothed log-weights of step t (rows = the
 * locations, cols = the particles of step t+1, col_a = the smoothed log-weights of step t+1, col_sub = den, row_add =
 * log_w_t).  The Normal's normalising constant cancels between the two and is never formed; so does a constant in log_w_t.
 * T is float32 or float64 (`dtype`); D == 0 (rows / cols / scale may be NULL) means no distance term.  All arithmetic is
 * in float64 whatever T is:
 *   inv[d]    = 1 / (double)scale[d]
 *   q[r,c]    = sum_d (((double)rows[b,r,d] - (double)cols[b,c,d]) * inv[d])^2          (d ascending)
 *   term[c]   = col_a[b,c] == -inf ? -inf : (double)col_a[b,c] - (double)col_sub[b,c]
 *   s[r,c]    = term[c] - 0.5 * q[r,c]
 *   out[b,r]  = (T)( (double)row_add[b,r] + (smax[r] + log sum_c exp(s[r,c] - smax[r])) ),   smax[r] = max_c s[r,c]
 * with K2's float64 exp of a non-positive number, and ONE rounding to T, at the end.  The order of the sum over c, the
 * reference value the exponentials are taken against while the maximum is not yet known, and the contraction of
 * multiply-adds are the kernel's: the result lies within
 *   2^-52 * ( (D + 4) * max_c (|term[c]| + q[r,c] / 2) + C + 8 )          (max over the columns with s[r,c] >= smax[r] - 40)
 * of the exact value (aesmc_amd/testing/smoothing.py: pairwise_lse_bound), before the rounding to T.
 * Special values, per (b, r); row points and batch rows never affect one another:
 *   a NaN among s[r,:] (from any operand, `scale` included) or in row_add[b,r]: AESMC_FLAG_NAN_LOG_WEIGHT, out = NaN;
 *   else smax[r] == +inf (a col_sub of -inf under a present column: a denominator without mass): AESMC_FLAG_DEGENERATE_ROW,
 *        out = +inf;
 *   else smax[r] == -inf (every column absent or infinitely far): out = -inf and NO flag — a point of zero weight.
 * No workspace; R and C are independent and not bounded by LDS.  D above 256 or R, C above 2^30 - 1 return
 * AESMC_ERR_UNSUPPORTED and launch nothing; B R == 0 is a no-op; C == 0 with row points to sum for is
 * AESMC_ERR_INVALID_ARGUMENT.
 */
int aesmc_pairwise_lse(int dtype, const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale,
                       int64_t scale_stride, const void *col_a, const void *col_sub, const void *row_add, void *out,
                       int32_t *flags, int64_t B, int64_t R, int64_t C, int64_t D, void *stream);

/* K23 — a pairwise Gaussian softmax mean: the building block of the two-slice particle smoother, which gives
 * E[g(x_{t+1}) f(x_t)^T | y_0..y_{T-1}] (the lag-one cross moment of an EM M-step, the statistic of a Fisher-identity
 * score) from the particles the filter stored.  The reference has no such call site.  With K22's operands and scores
 * s[r,c] (above), for every batch row b and row point r:
 *   out[b,r,p] = sum_c softmax_c(s[r,:])[c] * payload[b,c,p]
 *   lse[b,r]   = what aesmc_pairwise_lse writes for the same operands, bit for bit
 *   payload  T [B,C,P] view               `stride_k` steps along c, `stride_d` along p
 *   out      T [B,R,P] dense
 *   lse_out  T [B,R] dense or NULL
 * One backward step of the two-slice smoother is one launch of K23 (rows = the particles of step t+1, cols = the
 * transition's locations of step t's particles, col_a = log_w_t, payload = f(x_t): m[j] = the mean of f under the backward
 * kernel of particle j, lse = the denominators den[j]), one of K22 (the smoothed log-weights of step t, as above) and
 * the contraction sum_j w[t+1|T][j] g(x[t+1][j]) m[j]^T, which is the caller's.
 * All arithmetic is in float64 whatever T is, with K2's float64 exp of a non-positive number:
 *   e[r,c]     = exp(s[r,c] - smax[r]),   payload0[c,p] = col_a[b,c] == -inf ? 0 : (double)payload[b,c,p]
 *   out[b,r,p] = (T)( (sum_c e[r,c] * payload0[c,p]) / (sum_c e[r,c]) )
 * ONE rounding to T, at the end.  The order of the sums over c and the reference value the exponentials are taken against
 * while the maximum is not yet known are the kernel's: the result lies within
 *   2 * lse_bound[b,r] * sum_c softmax_c(s[r,:])[c] * |payload0[c,p]|        (lse_bound: K22's, above)
 * of the exact value (aesmc_amd/testing/smoothing.py: pairwise_mean_bound), before the rounding to T.
 * Special values, per (b, r); row points and batch rows never affect one another:
 *   an absent column (col_a == -inf) never reaches a result whatever its payload holds (NaN, inf): it is selected out,
 *        not multiplied by zero.  The payload of a PRESENT column must be finite;
 *   a NaN among s[r,:] or in row_add[b,r]: AESMC_FLAG_NAN_LOG_WEIGHT, out[b,r,:] = NaN and lse = NaN;
 *   else smax[r] == +inf: AESMC_FLAG_DEGENERATE_ROW, lse = +inf and out[b,r,:] = NaN (no weights to average with);
 *   else smax[r] == -inf: out[b,r,:] = 0, lse = -inf and NO flag — a point of zero weight.
 * No workspace.  D above 256, P above 256 or R, C above 2^30 - 1 return AESMC_ERR_UNSUPPORTED and launch nothing; P < 1
 * and a NULL payload / out are AESMC_ERR_INVALID_ARGUMENT; B R == 0 is a no-op; C == 0 with row points to average for is
 * AESMC_ERR_INVALID_ARGUMENT.  Every check runs before any launch.
 */
int aesmc_pairwise_mean(int dtype, const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale,
                        int64_t scale_stride, const void *col_a, const void *col_sub, const void *row_add,
                        const aesmc_view3 *payload, void *out, void *lse_out, int32_t *flags, int64_t B, int64_t R,
                        int64_t C, int64_t D, int64_t P, void *stream);

/* K24 — a pairwise Gaussian max and argmax: the building block of the MAP trajectory (the particle Viterbi recursion of
 * Godsill, Doucet & West 2001), which finds the single most probable path through the particles the filter stored.  The
 * reference has no such call site.  With K22's operands and scores s[r,c] (above: term[c] is -inf where col_a == -inf
 * whatever col_sub holds, D == 0 means no distance term, all arithmetic in float64 whatever T is), for every batch row b
 * and row point r:
 *   out[b,r] = (T)( (double)row_add[b,r] + smax[r] ),   smax[r] = max_c s[r,c]
 *   arg[b,r] = min{ c : s[r,c] == smax[r] }
 *   out      T [B,R] dense
 *   arg      int64 [B,R] dense or NULL    NULL: the maximum only
 * Ties go to the SMALLEST column index, exactly: every column's score chain is independent of its neighbours, so columns
 * with identical operands have identical bits.
 * One step of the recursion is one launch (rows = the particles of step t, cols = the transition's locations of step
 * t-1's particles, col_a = delta[t-1], row_add = the emission's log-density plus the transition's normalising constant:
 * out = delta[t], arg = psi[t]); a launch with D == 0 and one row point is the maximum of col_a and its smallest index.
 * ONE rounding to T, at the end.  The contraction of multiply-adds and the order of the D additions are the kernel's: the
 * result lies within
 *   2^-52 * ( (D + 4) * max_c (|term[c]| + q[r,c] / 2) + 4 + |out[b,r]| )     (max over the columns with s[r,c] >= smax[r] - 1)
 * of the exact value (aesmc_amd/testing/smoothing.py: pairwise_argmax_bound), before the rounding to T.
 * Special values, per (b, r); row points and batch rows never affect one another; arg == C means "no column" (K21's
 * convention for idx == K):
 *   a NaN among s[r,:] (from any operand, `scale` included) or in row_add[b,r]: AESMC_FLAG_NAN_LOG_WEIGHT, out = NaN, arg = C;
 *   else smax[r] == +inf: AESMC_FLAG_DEGENERATE_ROW, out = +inf, arg = C;
 *   else smax[r] == -inf (every column absent or infinitely far): out = -inf, arg = C and NO flag.
 * No workspace; R and C are independent and not bounded by LDS.  D above 256 or R, C above 2^30 - 1 return
 * AESMC_ERR_UNSUPPORTED and launch nothing; B R == 0 is a no-op; C == 0 with row points to maximise for is
 * AESMC_ERR_INVALID_ARGUMENT.
 */
int aesmc_pairwise_argmax(int dtype, const aesmc_view3 *rows, const aesmc_view3 *cols, const void *scale,
                          int64_t scale_stride, const void *col_a, const void *col_sub, const void *row_add, void *out,
                          int64_t *arg, int32_t *flags, int64_t B, int64_t R, int64_t C, int64_t D, void *stream);

/* K25 — a pairwise Gaussian weighted pass: the backward of K22, and through it of the marginal particle filter's
 * log-weights (Klaas, de Freitas & Doucet 2005; as a training objective: Lai, Domke & Sheldon 2022).  The reference has no
 * such call site.  `own` are the points a result belongs to, `others` the points summed over.  For every batch row b and
 * own point n:
 *   w[n,m]        = exp( own_term[b,n] + other_term[b,m] - 1/2 sum_d ((own[b,n,d] - others[b,m,d]) / scale[d])^2 )
 *                   * own_gain[b,n] * other_gain[b,m]
 *   mass[b,n]     = sum_m w[n,m]
 *   pull[b,n,d]   = sum_m w[n,m] * (others[b,m,d] - own[b,n,d]) / scale[d]^2
 *   spread[b,n,d] = sum_m w[n,m] * ((own[b,n,d] - others[b,m,d]) / scale[d])^2
 *   own         T [B,N,D] view              `stride_k` steps along n
 *   others      T [B,M,D] view              `stride_k` steps along m
 *   scale       T, D values                 read with the element stride `scale_stride`: 0 (one value) or 1
 *   own_term    T [B,N] dense               not finite: the own point gets zeros and no flag
 *   other_term  T [B,M] dense               -inf: the other is absent
 *   own_gain    T [B,N] dense or NULL       NULL: 1
 *   other_gain  T [B,M] dense or NULL       NULL: 1
 *   mass        T [B,N] dense or NULL
 *   pull        T [B,N,D] dense or NULL
 *   spread      T [B,N,D] dense or NULL
 * With L = out - row_add of a K22 launch, term = col_a - col_sub (-inf where col_a is -inf) and g the gradient arriving at
 * `out`, K22's backward is two launches.  The row points own the columns (own_term = -L, other_term = term, own_gain = g):
 * grad_rows = pull, grad_scale[d] = sum_{b,r} spread[b,r,d] / scale[d] (the caller's reduction), mass = g.  The columns own
 * the row points (own_term = term, other_term = -L, -inf where L is not finite, other_gain = g): grad_col_a = mass,
 * grad_col_sub = -mass, grad_cols = pull.  grad_row_add = g.  The normaliser is an operand: every exponent of a finite own
 * point is <= about 0, nothing is rescaled.
 * T is float32 or float64 (`dtype`); D == 0 (own / others / scale may be NULL) means no distance term and `mass` alone.  All
 * arithmetic is in float64 whatever T is, the exponent K22's chain (inv[d] = 1 / (double)scale[d], d ascending), the
 * sums formed from the differences (own - others) * inv, never from raw moments, with K2's float64 exp, and ONE rounding
 * to T, at the end.  The order of the sums over m and the contraction of multiply-adds are the kernel's: every output
 * X = sum_m t_m lies within
 *   2^-52 * ( (D + 4) * max_m (|own_term| + |other_term[m]| + q[n,m] / 2) + M + 16 ) * sum_m |t_m|
 * (max over the others whose exponent is within 40 of the own point's largest) of the exact value, plus the floor that
 * float64's gradual underflow below 2^-1022 sets (aesmc_amd/testing/marginal_filter.py: pairwise_pass_bound), before the
 * rounding to T.
 * Special values, per (b, n); own points and batch rows never affect one another:
 *   an absent other (other_term == -inf) never reaches a result whatever it holds (NaN, inf): it is selected out, not
 *        multiplied by zero.  The coordinates of a PRESENT other and of an own point with a finite own_term are finite or NaN;
 *   own_term not finite (-inf: an absent column; +inf, NaN: a row point whose forward value was -inf, +inf or NaN, and
 *        which K22 has flagged where there was something to flag): mass, pull, spread = 0 and NO flag;
 *   else a NaN or +inf exponent, or a NaN weight, against a present other (a NaN other_term, coordinate, scale or gain):
 *        AESMC_FLAG_NAN_LOG_WEIGHT, and mass, pull, spread of that own point = NaN.
 * No workspace, no atomics; N and M are independent and not bounded by LDS.  D above 256 or N, M above 2^30 - 1 return
 * AESMC_ERR_UNSUPPORTED and launch nothing; NULL terms, no output to write (mass NULL and, for D > 0, pull and spread NULL
 * too) are AESMC_ERR_INVALID_ARGUMENT; B N == 0 is a no-op; M == 0 with own points to sum for is
 * AESMC_ERR_INVALID_ARGUMENT.  Every check runs before any launch.
 */
int aesmc_pairwise_pass(int dtype, const aesmc_view3 *own, const aesmc_view3 *others, const void *scale,
                        int64_t scale_stride, const void *own_term, const void *other_term, const void *own_gain,
                        const void *other_gain, void *mass, void *pull, void *spread, int32_t *flags, int64_t B,
                        int64_t N, int64_t M, int64_t D, void *stream);

/* K26 — conditional multinomial resampling with ancestor sampling: the ancestors of one step of conditional SMC
 * (particle Gibbs; Andrieu, Doucet & Holenstein 2010) whose slot K-1 carries a reference path, that slot's ancestor being
 * drawn anew given the reference's next state (PGAS; Lindsten, Jordan & Schoen 2014).  The reference has no such call
 * site.  Systematic and stratified resampling (K2) have no simple exact conditional form (Chopin & Singh 2015);
 * multinomial resampling has, and this is it.  Per batch row, in one launch:
 *   log_w   T [B,K] dense                 the step's log-weights
 *   u       float64 [B,K] dense           in [0, 1), one uniform per slot
 *   loc     T [B,K,D] view                the transition's location for every particle
 *   target  T [B,1,D] view                the reference path's next state (`stride_k` is not read)
 *   scale   T, D values                   read with the element stride `scale_stride`: 0 (one value) or 1
 * All arithmetic is in float64 whatever T is (float32 or float64, `dtype`):
 *   w[j]       = exp(log_w[b,j] - max_j log_w[b,:])                      (K2's float64 exp of a non-positive number)
 *   C[j]       = w[0] + ... + w[j]                                       (added front to back, one at a time)
 *   idx[b,k]   = min( #{j : C[j] <= u[b,k] * C[K-1]},  max{j : w[j] > 0} )               k = 0 .. K-2
 *   idx[b,K-1] = K - 1                                                                   D == 0: no transition term
 *   idx[b,K-1] = the same formula over s[j] = log_w[b,j] - 1/2 sum_d ((target[b,d] - loc[b,j,d]) * inv[d])^2, inv[d] =
 *                1 / (double)scale[d], at u[b,K-1]: K21's score and draw for ONE trajectory (d ascending, the scaled
 *                difference squared into a fused multiply-add).
 * The free slots are K21's draw without a transition term at u[:, :K-1], the pinned slot K21's with M = 1.  Unlike K21's,
 * the sums C are formed strictly front to back, so the index does not depend on an association of the additions.
 * Bad rows, by K2's conventions: a NaN among log_w[b,:] raises AESMC_FLAG_NAN_LOG_WEIGHT, a maximum that is not finite
 * AESMC_FLAG_DEGENERATE_ROW, and every slot of the row is K; a NaN among s (from loc or target) or no finite maximum of s
 * raises the same flags and only idx[b,K-1] = K.  K == 1 gives idx = 0.
 * The CDFs live in LDS: K above 8192 or D above 256 return AESMC_ERR_UNSUPPORTED and launch nothing; B K == 0 is a no-op.
 * No workspace.  Every check runs before any launch.
 */
int aesmc_conditional_ancestor_index(int dtype, const void *log_w, const double *u, const aesmc_view3 *loc,
                                     const aesmc_view3 *target, const void *scale, int64_t scale_stride, int64_t *out_idx,
                                     int32_t *flags, int64_t B, int64_t K, int64_t D, void *stream);

/* K27 — the first-stage log-weights of a fully adapted auxiliary particle filter (Pitt & Shephard 1999): for a Normal
 * transition N(mu, S_f) with a constant diagonal S_f and an emission N(C x + d, S_g), the predictive likelihood
 *   out[b,k] = base - 1/2 || P mu[b,k] + o_b ||^2  =  log p(y_t | x_{t-1}[b,k]),
 * P = -W C, o_b = W (y_b - d_b), W the inverse Cholesky factor of S = C S_f C^T + S_g, base = -Dy/2 log 2 pi - log det
 * chol(S): small float64 operands the host forms once.  The reference has no such call site.
 *   loc     T [B,K,D] view by element strides (0 = broadcast)      the transition's location mu for every particle
 *   P       float64 [Dy,D] dense
 *   offset  float64 [B,Dy] dense
 *   out     T [B,K] dense
 * All arithmetic is in float64 whatever T is (float32 or float64, `dtype`):
 *   r_j      = one chain of fused multiply-adds over i = 0 .. D-1 ascending, starting from offset[b,j], of
 *              P[j,i] * (double)loc[b,k,i]
 *   q        = one chain over j = 0 .. Dy-1 ascending, starting from 0, of r_j * r_j
 *   out[b,k] = (T)(base - 0.5 q)
 * A NaN location gives a NaN log-weight and nothing else: the resampling launch that follows raises
 * AESMC_FLAG_NAN_LOG_WEIGHT by its own rules, so this entry takes no flags.
 * D and Dy lie in 1 .. aesmc_affine_max_dim(); beyond that, or B K beyond 32-bit element arithmetic, the entry returns
 * AESMC_ERR_UNSUPPORTED and launches nothing.  NULL pointers, negative sizes, D or Dy below 1 and a base not aligned to
 * its element return AESMC_ERR_INVALID_ARGUMENT.  B K == 0 is a no-op.  Every check runs before any launch.
 */
int aesmc_affine_quadratic_logweight(int dtype, const aesmc_view3 *loc, const double *P, const double *offset, double base,
                                     void *out, int64_t B, int64_t K, int64_t D, int64_t Dy, void *stream);

/* K28 — the draw of a fully adapted auxiliary particle filter step: the optimal proposal p(x_t | x_{t-1}, y_t) =
 * N(r_b + M mu, L L^T) with its full covariance, through the ancestors the resampling launch drew from K27's weights.
 * M = I - G C, r_b = G (y_b - d_b), G = S_f C^T S^-1 the gain, L the Cholesky factor of S_f - G C S_f.
 *   loc     T [B,K,D] view by element strides (0 = broadcast)      the transition's location for every STORED particle
 *   idx     int64 [B,K] dense, or NULL for the identity; NOT assumed sorted
 *   M, L    float64 [D,D] dense; of L only L[j,i] with i <= j is read
 *   offset  float64 [B,D] dense
 *   eps     T [B,K,D] dense, 16-byte aligned                       standard-normal noise
 *   out     T [B,K,D] dense, 16-byte aligned; must not alias an input
 * With a = idx ? idx[b,k] : k, out[b,k,j] is ONE chain of float64 fused multiply-adds rounded once to T, in this order:
 *   start from offset[b,j];
 *   add M[j,i] * (double)loc[b,a,i]   for i = 0 .. D-1;
 *   add L[j,i] * (double)eps[b,k,i]   for i = 0 .. j.
 * An `a` outside [0, K) reads nothing, writes NaN to that particle's D values and raises AESMC_FLAG_INDEX_OUT_OF_RANGE
 * (K2 marks a flagged row with idx == K).
 * D lies in 1 .. aesmc_affine_max_dim(); sizes, statuses and the no-op as K27's.
 */
int aesmc_adapted_draw(int dtype, const aesmc_view3 *loc, const int64_t *idx, const double *M, const double *offset,
                       const double *L, const void *eps, void *out, int32_t *flags, int64_t B, int64_t K, int64_t D,
                       void *stream);

/* Bytes of workspace K29 / K30 need for these extents (float64 partial sums: a fixed block for the matrices, 256 bytes
 * per 64 particles for the batch rows' sums); 0 for extents the entries do not launch for. */
int64_t aesmc_adapted_backward_workspace_bytes(int64_t B, int64_t K, int64_t D, int64_t Dy);

/* K29 — the adjoint of K27.  With rho[b,k,j] = offset[b,j] + sum_i P[j,i] loc[b,k,i] evaluated by K27's own chain and
 * w[b,k,j] = -(grad[b,k] * rho[b,k,j]) (one rounding, float64):
 *   grad_loc[b,k,i]   = sum_j w[b,k,j] P[j,i]        T [B,K,D] dense, 16-byte aligned: ONE chain of float64 fused
 *                                                    multiply-adds over j = 0 .. Dy-1 ascending from zero, rounded once
 *   grad_P[j,i]       = sum_{b,k} w[b,k,j] loc[b,k,i]  float64 [Dy,D]
 *   grad_offset[b,j]  = sum_k w[b,k,j]                 float64 [B,Dy]
 * (the gradient of `base` is the sum of grad: the caller's).  loc, P, offset as K27 takes them; grad T [B,K] dense.
 * Each of the three outputs may be NULL (not wanted, not computed); all three NULL is an invalid argument.
 * The two reductions use no floating-point atomics and one fixed order of additions for given extents — the float64
 * matrix cores over each wavefront's 64 particles, the wavefronts of a workgroup in order, the workgroups (batch rows:
 * the 64-particle chunks) in order in a second launch: the same operands give the same bits.
 * workspace: aesmc_adapted_backward_workspace_bytes(B, K, D, Dy) bytes, 8-byte aligned; needed unless grad_P and
 * grad_offset are both NULL.  Sizes, statuses and the no-op as K27's; an output that aliases its input is an invalid
 * argument.  Every check runs before any launch.
 */
int aesmc_affine_quadratic_logweight_backward(int dtype, const aesmc_view3 *loc, const double *P, const double *offset,
                                              const void *grad, void *grad_loc, double *grad_P, double *grad_offset,
                                              void *workspace, int64_t workspace_bytes, int64_t B, int64_t K, int64_t D,
                                              int64_t Dy, void *stream);

/* K30 — the adjoint of K28 for the gradient `grad` T [B,K,D] (dense, 16-byte aligned) arriving at its output.  With
 * a = idx ? idx[b,k] : k:
 *   h[b,k,i]      = sum_j grad[b,k,j] M[j,i]             T [B,K,D] dense, 16-byte aligned: ONE chain over j = 0 .. D-1
 *                                                        ascending from zero, rounded once — the gradient of the
 *                                                        GATHERED row loc[b,a,:]; summing it over equal ancestors
 *                                                        (aesmc_resample_gather_backward) is the caller's
 *   grad_M[j,i]   = sum_{b,k} grad[b,k,j] loc[b,a,i]     float64 [D,D]
 *   grad_L[j,i]   = sum_{b,k} grad[b,k,j] eps[b,k,i]     float64 [D,D] for i <= j; exactly 0 above the diagonal
 *   grad_r[b,j]   = sum_k grad[b,k,j]                    float64 [B,D]  (the gradient of K28's `offset`)
 * Each of the four outputs may be NULL; all four NULL is an invalid argument.  L's values are not needed.  An `a` outside
 * [0, K) reads nothing and contributes nothing to the three sums; that particle's h row is NaN and
 * AESMC_FLAG_INDEX_OUT_OF_RANGE is raised.  Reductions, workspace, sizes and statuses as K29's.
 */
int aesmc_adapted_draw_backward(int dtype, const aesmc_view3 *loc, const int64_t *idx, const double *M, const void *eps,
                                const void *grad, void *h, double *grad_M, double *grad_L, double *grad_r, int32_t *flags,
                                void *workspace, int64_t workspace_bytes, int64_t B, int64_t K, int64_t D, void *stream);

/* K31 — one step of the Rao-Blackwellised particle filter (mixture Kalman filter; Doucet, de Freitas, Murphy & Russell
 * 2000; Chen & Liu 2000) for a switching linear-Gaussian state-space model with M regimes, latent z in R^D, observation
 * y in R^Dy:
 *   s_0 ~ Cat(pi0)              s_t | s_{t-1} ~ Cat(Pi[s_{t-1},:])
 *   z_0 ~ N(m0, diag(s0^2))     z_t = A[s_t] z_{t-1} + b[s_t] + N(0, diag(q[s_t]^2))
 *   y_t = C[s_t] z_t + d[s_t] + N(0, diag(r[s_t]^2))                      (also at t = 0, under s_0)
 * Only the regimes are sampled: particle (b,k) carries its regime s, and the exact Kalman mean m and covariance P of z
 * given its regime history; its weight is the Kalman predictive likelihood.  The reference has no such call site.
 * The model, all float64, dense, 8-byte aligned (the host expands anything shared across regimes): */
typedef struct {
  const double *cdf0;      /* [M]    cumulative pi0, last entry 1: read by the step-0 form only                     */
  const double *cdf;       /* [M,M]  cumulative rows of Pi, last entry of each 1: read by the later form only       */
  const double *m0, *s0;   /* [D]    the initial mean and scale: read by the step-0 form only                       */
  const double *A, *b, *q; /* [M,D,D], [M,D], [M,D]                                                                 */
  const double *C, *d, *r; /* [M,Dy,D], [M,Dy], [M,Dy]                                                              */
  int64_t M, D, Dy;
} aesmc_switching_model;
/*   regime_in   int32 [B,K], mean_in float64 [B,K,D], cov_in float64 [B,K,D(D+1)/2]: the STORED particles of the step
 *               before — all three NULL: the step-0 form, which reads no state and no idx; cov is the packed lower
 *               triangle, element (i,j) with i >= j at i(i+1)/2 + j
 *   idx         int64 [B,K] dense, or NULL for the identity; NOT assumed sorted
 *   uniforms    float64 [B,K]                       y   T [B,Dy] dense, T float32 or float64 (`y_dtype`), widened on read
 *   regime_out, mean_out, cov_out as the inputs, log_weight float64 [B,K]: written out of place (the gather forbids in
 *               place: an output that is its own input is an invalid argument)
 * Per particle, with j = idx ? idx[b,k] : k (step 0: k), everything in float64, every sum ONE chain of fused multiply-adds
 * in ascending index order starting from the value named first:
 *   s        = #{ i < M-1 : cdf[regime_in[b,j], i] <= uniforms[b,k] }                 (step 0: the row cdf0)
 *   m-_i     = b_s[i] + sum_l A_s[i,l] m[b,j,l]                                          (step 0: m0)
 *   W_il     = 0 + sum_c A_s[i,c] P[b,j][c,l];   P-_ij = (i == j ? q_s[i]^2 : 0) + sum_l A_s[i,l] W_jl,  i >= j
 *                                                                                        (step 0: diag(s0^2))
 *   e_i      = (y[b,i] - d_s[i]) - sum_l C_s[i,l] m-_l
 *   U_il     = 0 + sum_c C_s[i,c] P-[c,l];       S_ij = (i == j ? r_s[i]^2 : 0) + sum_l C_s[i,l] U_jl,    i >= j
 *   Lam      = chol(S) column by column: Lam_jj = sqrt(S_jj - sum_{c<j} Lam_jc^2), rho_j = 1 / Lam_jj,
 *              Lam_ij = (S_ij - sum_{c<j} Lam_ic Lam_jc) rho_j
 *   v_i      = (e_i - sum_{c<i} Lam_ic v_c) rho_i;   V_il = (U_il - sum_{c<i} Lam_ic V_cl) rho_i
 *   log_weight[b,k] = (-1/2 sum_i v_i^2 - sum_j log Lam_jj) - Dy * (1/2 log 2 pi)
 *   mean_out_l = m-_l + sum_i V_il v_i;          cov_out_lj = P-_lj - sum_i V_il V_ij,  l >= j (the lower triangle only)
 * An idx outside [0, K) or a stored regime outside [0, M) reads nothing further, writes regime 0 and NaN to the particle's
 * mean, covariance and log-weight and raises AESMC_FLAG_INDEX_OUT_OF_RANGE.  A pivot S_jj - sum that is not positive
 * writes the drawn regime and NaN to the particle's mean, covariance and log-weight; the resampling launch that follows
 * raises AESMC_FLAG_NAN_LOG_WEIGHT by its own rules.
 * NULL or misaligned pointers, negative sizes, M, D or Dy below 1, an unknown dtype, a state given in part and an output
 * that aliases its input return AESMC_ERR_INVALID_ARGUMENT; B K == 0 is a no-op; D above aesmc_switching_max_latent_dim(),
 * Dy above aesmc_switching_max_observation_dim(), M above aesmc_switching_max_regimes() or B K beyond 32-bit element
 * arithmetic return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch.  `flags` may be NULL. */
int64_t aesmc_switching_max_latent_dim(void);      /* 8 */
int64_t aesmc_switching_max_observation_dim(void); /* 8 */
int64_t aesmc_switching_max_regimes(void);         /* 16 */
int aesmc_switching_kalman_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                const double *mean_in, const double *cov_in, const int64_t *idx, const double *uniforms,
                                const void *y, int32_t *regime_out, double *mean_out, double *cov_out, double *log_weight,
                                int32_t *flags, int64_t B, int64_t K, void *stream);

/* K32 — the look-ahead of the fully adapted filter of the same model (the mixture Kalman filter with the regimes drawn from
 * their exact posterior: Chen & Liu 2000; Doucet, Gordon & Krishnamurthy 2001; Pitt & Shephard 1999): for the STORED particle
 * (b,k) — no ancestors — one Kalman prediction per regime j = 0..M-1, each K31's arithmetic up to v under s = j:
 *   l_j   = (-1/2 sum_i v_i^2 - sum_c log Lam_cc) - Dy * (1/2 log 2 pi)
 *   g_j   = log_prior[regime_in[b,k], j] + l_j  (one rounded addition; step 0: log_prior[j]); -inf where the log-prior is
 *           -inf whatever l_j and its pivots are; NaN where the log-prior is finite and a pivot is not positive
 *   log_weight[b,k] = top + log(sum_j exp(g_j - top)), top = max_j g_j, the sum from 0 in ascending j
 *   cdf[b,k,j]      = sum_{i <= j} exp(g_i - log_weight[b,k]) from 0 in ascending i; exactly 1 for every j from the last i
 *                     with exp(g_i - log_weight) > 0 onwards
 *   log_prior   float64 [M,M] with a state (rows: from-regime), [M] without one: the logarithms of Pi or pi0, -inf allowed
 *   regime_in, mean_in, cov_in, y, flags as K31's (all three state pointers NULL: the step-0 form, every regime predicted
 *               by m0 and diag(s0^2)); the model's cdf0 and cdf are not read
 *   log_weight  float64 [B,K], cdf float64 [B,K,M]
 * A stored regime outside [0, M) writes NaN to the particle's log-weight and CDF row and raises
 * AESMC_FLAG_INDEX_OUT_OF_RANGE.  A NaN score, or no score above -inf, writes NaN to both (the resampling launch that
 * follows raises AESMC_FLAG_NAN_LOG_WEIGHT by its own rules).  Statuses as K31's; an output that is another operand is an
 * invalid argument. */
int aesmc_switching_lookahead(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                              const int32_t *regime_in, const double *mean_in, const double *cov_in, const void *y,
                              double *log_weight, double *cdf, int32_t *flags, int64_t B, int64_t K, void *stream);

/* K33 — K31 with the regime drawn from a cumulative row per particle: with j the ancestor as in K31 (step 0: k),
 *   s = #{ i < M-1 : particle_cdf[b,j,i] <= uniforms[b,k] }
 * and everything after it K31's, in K31's order; log_weight receives l_s, which the adapted filter does not use (it equals
 * K32's g_s - log_prior[., s] to rounding).  particle_cdf: float64 [B,K,M] (K32's cdf), must not be an output; the model's
 * cdf0 and cdf are not read.  Everything else, the conventions and the statuses as K31's. */
int aesmc_switching_kalman_draw(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                const double *mean_in, const double *cov_in, const int64_t *idx, const double *uniforms,
                                const double *particle_cdf, const void *y, int32_t *regime_out, double *mean_out,
                                double *cov_out, double *log_weight, int32_t *flags, int64_t B, int64_t K, void *stream);

/* K34 — the information step of Rao-Blackwellised backward simulation for the same model (Fong, Godsill, Doucet & West
 * 2002; Whiteley, Andrieu & Doucet 2010; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016).  Trajectory (b,n) carries, for its
 * future regimes, p(y_{t+1..T-1} | z_t) = exp(c + lam^T z_t - 1/2 z_t^T Om z_t); the call takes (Om, lam, c) of time t+1 to
 * time t.  With j = regime_next[b,n] (the trajectory's regime at t+1), y the observation of time t+1, r2_i = r_j[i]^2,
 * q2_i = q_j[i]^2, sq_i = sqrt(q2_i); float64, every sum ONE chain of fused multiply-adds in ascending index order starting
 * from the value named first; symmetric matrices and the factor as packed lower triangles, (i,k) with i >= k at i(i+1)/2 + k:
 *   e_i    = y[b,i] - d_j[i];  rho_i = 1 / r2_i;  G_il = C_j[i,l] rho_i
 *   Oh_pq  = Om_pq + sum_i G_ip C_j[i,q];   lh_p = lam_p + sum_i G_ip e_i
 *   ch     = ((c - 1/2 sum_i (e_i rho_i) e_i) - 1/2 sum_i log r2_i) - Dy * (1/2 log 2 pi)
 *   Mm_pq  = (p == q) + (sq_p sq_q) Oh_pq;  L = chol(Mm) column by column as K31's Lam (the pivots are at least 1)
 *   X_il   = (sq_i Oh_il - sum_{c<i} L_ic X_cl) / L_ii;   w_i = (sq_i lh_i - sum_{c<i} L_ic w_c) / L_ii
 *   Ot_pq  = Oh_pq - sum_i X_ip X_iq;       g_p = lh_p - sum_i X_ip w_i
 *   ob_p   = 0 + sum_l Ot_pl b_j[l]
 *   omega_out_pq  = 0 + sum_i A_j[i,p] (0 + sum_c Ot_ic A_j[c,q]);      lambda_out_p = 0 + sum_i A_j[i,p] (g_i - ob_i)
 *   c_out  = (((ch - sum_i log L_ii) + 1/2 sum_i w_i^2) + sum_i b_j[i] g_i) - sum_i (1/2 b_j[i]) ob_i
 *   factor_out F: the lower factor of omega_out (F F^T = omega_out; Phi = F^T is upper-triangular with Phi^T Phi = omega_out),
 *            column by column with tau = 2^-40 max_i omega_out_ii: p_k = omega_out_kk - sum_{c<k} F_kc^2; where p_k <= tau
 *            (or is NaN) column k of F is ZERO, otherwise F_kk = sqrt(p_k), F_ik = (omega_out_ik - sum_{c<k} F_ic F_kc) / F_kk
 *            — omega_out is only positive SEMI-definite (rank <= Dy at t = T-2)
 *   regime_next int32 [B,N];  omega_in float64 [B,N,D(D+1)/2], lambda_in float64 [B,N,D], c_in float64 [B,N] — all three NULL:
 *               the zeros of the last step;  y T [B,Dy] (`y_dtype`);  the outputs as the inputs, factor_out as omega_out,
 *               out of place;  the model's cdf0, cdf, m0 and s0 are not read
 * A regime outside [0, M) writes NaN to the trajectory's four outputs and raises AESMC_FLAG_INDEX_OUT_OF_RANGE.
 * NULL or misaligned pointers, negative sizes, M, D or Dy below 1, an unknown dtype, an input given in part and an output
 * that is another operand return AESMC_ERR_INVALID_ARGUMENT; B N == 0 is a no-op; D, Dy or M above the limits of K31 or B N
 * beyond 32-bit element arithmetic return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch.  `flags` may be NULL. */
int aesmc_switching_information_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_next,
                                     const double *omega_in, const double *lambda_in, const double *c_in, const void *y,
                                     double *omega_out, double *lambda_out, double *c_out, double *factor_out,
                                     int32_t *flags, int64_t B, int64_t N, void *stream);

/* K35 — the pair scores of that backward simulation: for trajectory (b,n) with K34's F and lam of time t and stored particle
 * (b,k) of step t with regime s, mean m, packed covariance P and log-weight log w, the logarithm of w Pi[s, s'] times the
 * integral of exp(lam^T z - 1/2 z^T Om z) against N(m, P) (the trajectory's c is left out: it does not change the draw).
 * Only F and lam are read (Om m = F (F^T m)); chains as K34's:
 *   t_i = 0 + sum_{l>=i} F_li m_l;   mq = 0 + sum_i t_i^2;   h_l = lam_l - sum_{i<=l} F_li t_i;   lm = 0 + sum_l lam_l m_l
 *   hph = 0 + sum_c h_c (0 + sum_l P_cl h_l)
 *   W_il = 0 + sum_{c>=i} F_ci P_cl;  v_i = 0 + sum_l W_il h_l;  Lam_ij = (i == j) + sum_{l>=j} W_il F_lj,  j <= i
 *   G = chol(Lam) as K31's (the pivots are at least 1: no test, no flag);  x_i = (v_i - sum_{c<i} G_ic x_c) / G_ii
 *   scores[b,n,k] = ((((log_w[b,k] + log_Pi[s, s']) + lm) - 1/2 mq) + 1/2 (hph - sum_i x_i^2)) - sum_i log G_ii
 *                   and -inf where log_Pi[s, s'] is -inf, whatever the rest is
 *   log_Pi float64 [M,M] (rows: from-regime; -inf allowed);  regime_next int32 [B,N];  factor float64 [B,N,D(D+1)/2], lambda
 *   float64 [B,N,D];  regime int32 [B,K], mean float64 [B,K,D], cov float64 [B,K,D(D+1)/2];  log_w float64 [B,K] or NULL
 *   (equal weights: nothing is added);  scores float64 [B,N,K]
 * A regime outside [0, M) on either side writes NaN and raises AESMC_FLAG_INDEX_OUT_OF_RANGE.  P is never factored: P = 0
 * is fine.  NULL (but log_w, flags) or misaligned pointers, negative sizes, M or D below 1 and scores being another operand
 * return AESMC_ERR_INVALID_ARGUMENT; B N == 0 or K == 0 is a no-op; D or M above the limits of K31 or B N K (or B K D(D+1)/2,
 * B N D(D+1)/2) beyond 32-bit element arithmetic return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch. */
int aesmc_switching_backward_scores(const double *log_Pi, const int32_t *regime_next, const double *factor,
                                    const double *lambda, const int32_t *regime, const double *mean, const double *cov,
                                    const double *log_w, double *scores, int32_t *flags, int64_t B, int64_t K, int64_t N,
                                    int64_t M, int64_t D, void *stream);

/* K36 — the two-filter combination of the state smoother of the same model (Fong, Godsill, Doucet & West 2002; Lindsten et
 * al. 2016).  Along a regime trajectory the model is linear-Gaussian: trajectory (b,n) has at time t the conditional Kalman
 * filter's mean m and packed covariance P (K31 under its regimes) and K34's F and lam of time t (Om = F F^T).  The call
 * writes the smoothed mean and packed covariance of z_t given ALL observations and the trajectory's regimes and, on
 * request, the lag-one cross-covariance.  No predicted covariance is inverted: q = 0 components and P = 0 are fine.
 * Chains as K34's (float64, every sum ONE chain of fused multiply-adds in ascending index order from the value named first):
 *   t_i  = 0 + sum_{l>=i} F_li m_l;   h_l = lam_l - sum_{i<=l} F_li t_i                                        (K35's t, h)
 *   W_il = 0 + sum_{c>=i} F_ci P_cl;  Lam_ij = (i == j) + sum_{l>=j} W_il F_lj,  j <= i                         (K35's W, Lam)
 *   G = chol(Lam) as K31's (the pivots are at least 1: no test, no flag);  U_il = (W_il - sum_{c<i} G_ic U_cl) / G_ii
 *   cov_out_pq  = P_pq - sum_i U_ip U_iq,  p >= q
 *   mean_out_p  = m_p + sum_l cov_out_pl h_l
 * and with cross_out, j = regime_next[b,n] (the trajectory's regime at t+1), r2_i = r_j[i]^2:
 *   rho_i = 1 / r2_i;  Gc_il = C_j[i,l] rho_i;  Oh_pq = omega_next_pq + sum_i Gc_ip C_j[i,q]                    (K34's Oh)
 *   V_il  = 0 + sum_c A_j[i,c] P_cl;   Y_pl = 0 + sum_q Oh_pq V_ql
 *   cross_out[b,n,i,l] = V_il - sum_p cov_next_ip Y_pl           = Cov(z_{t+1,i}, z_{t,l} | y_{0:T-1}, s_{0:T-1})
 * (divisions by a pivot are one reciprocal per pivot and a product, as K34's).
 *   mean float64 [B,N,D], cov float64 [B,N,D(D+1)/2], factor float64 [B,N,D(D+1)/2], lambda float64 [B,N,D]: of time t
 *   regime_next int32 [B,N];  omega_next float64 [B,N,D(D+1)/2]: K34's omega_out of time t+1, NULL at t+1 = T-1 (zeros);
 *   cov_next float64 [B,N,D(D+1)/2]: this call's cov_out of time t+1 (at t+1 = T-1 the filter's own covariance)
 *   mean_out, cov_out as mean, cov, out of place;  cross_out float64 [B,N,D,D] row-major, or NULL
 * Only the cross-covariance reads model (A, C, r of it; its D must be the argument D), regime_next, omega_next and cov_next:
 * with cross_out NULL all four MUST be NULL (an invalid argument otherwise: who hands them over expects a cross-covariance),
 * nothing of them is read and no regime is checked.  With cross_out a regime outside [0, M) writes NaN to the trajectory's
 * three outputs and raises AESMC_FLAG_INDEX_OUT_OF_RANGE.  NULL (but omega_next, flags, and the four above) or misaligned
 * pointers, negative sizes, D (with cross_out: M, Dy) below 1 and an output that is an input or another output return
 * AESMC_ERR_INVALID_ARGUMENT; B N == 0 is a no-op; D (with cross_out: Dy, M) above the limits of K31 or B N D^2 beyond 32-bit
 * element arithmetic return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch.  `flags` may be NULL. */
int aesmc_switching_smooth_combine(const aesmc_switching_model *model, const int32_t *regime_next, const double *mean,
                                   const double *cov, const double *factor, const double *lambda,
                                   const double *omega_next, const double *cov_next, double *mean_out, double *cov_out,
                                   double *cross_out, int32_t *flags, int64_t B, int64_t N, int64_t D, void *stream);

/* K37 — conditional multinomial resampling for the regimes of the same model: the ancestors of one step of a conditional
 * Rao-Blackwellised filter with ancestor sampling (particle Gibbs on the regimes; Whiteley, Andrieu & Doucet 2010; Lindsten,
 * Bunch, Saerkkae, Schoen & Godsill 2016).  K26 with the pinned slot's transition score replaced by K35's integral for the ONE
 * reference trajectory of the batch row.  Per batch row, in one launch, everything in float64:
 *   log_w   float64 [B,K]      the step's log-weights              u   float64 [B,K] in [0, 1), one uniform per slot
 *   log_Pi  float64 [M,M]      rows: from-regime, -inf allowed     regime_next int32 [B]: the reference's regime at the step
 *                                                                  being entered
 *   factor  float64 [B,D(D+1)/2], lambda float64 [B,D]: K34's factor_out and lambda_out with N = 1 along the reference
 *   regime  int32 [B,K], mean float64 [B,K,D], cov float64 [B,K,D(D+1)/2]: the stored particles the weights belong to
 *   w[j]       = exp(log_w[b,j] - max_j log_w[b,:]);  C[j] = w[0] + ... + w[j]  (added front to back, one at a time)
 *   idx[b,k]   = min( #{j : C[j] <= u[b,k] * C[K-1]},  max{j : w[j] > 0} )               k = 0 .. K-2: K26's, bit for bit
 *   idx[b,K-1] = the same formula at u[b,K-1] over s[j] = K35's scores[b,0,j] of particle j against (regime_next[b], factor[b],
 *                lambda[b]) with log_w[b,j] included — K35's chains in K35's order; -inf where log_Pi[regime[b,j],
 *                regime_next[b]] is -inf
 *   idx[b,K-1] = K - 1         factor and lambda both NULL (no ancestor sampling: log_Pi, regime_next and the stored
 *                              particles are not read and may be NULL)
 * Bad rows, by K26's conventions: a NaN among log_w[b,:] raises AESMC_FLAG_NAN_LOG_WEIGHT, a maximum that is not finite
 * AESMC_FLAG_DEGENERATE_ROW, and every slot of the row is K; a NaN among s or no finite maximum of s (every transition into
 * regime_next[b] has probability zero) raises the same flags and only idx[b,K-1] = K.  A stored regime or regime_next[b]
 * outside [0, M) gives NaN scores (and so the above) and raises AESMC_FLAG_INDEX_OUT_OF_RANGE.  K == 1 gives idx = 0.
 * The CDFs, and for D above 4 the covariances, live in LDS: K above aesmc_switching_conditional_max_particles(D) (8192 up to
 * D = 4, 4096 above; 0 for a D outside 1 .. aesmc_switching_max_latent_dim()), D or M above the limits of K31 or B K beyond
 * 32-bit element arithmetic return AESMC_ERR_UNSUPPORTED.  NULL (but flags; factor and lambda together; what they make
 * unread) or misaligned pointers, negative sizes, M or D below 1 and out_idx being another operand return
 * AESMC_ERR_INVALID_ARGUMENT; B K == 0 is a no-op.  No workspace.  Every check runs before any launch. */
int64_t aesmc_switching_conditional_max_particles(int64_t D);
int aesmc_switching_conditional_ancestor_index(const double *log_w, const double *u, const double *log_Pi,
                                               const int32_t *regime_next, const double *factor, const double *lambda,
                                               const int32_t *regime, const double *mean, const double *cov,
                                               int64_t *out_idx, int32_t *flags, int64_t B, int64_t K, int64_t M, int64_t D,
                                               void *stream);

/* K38 — K31 with the regime of slot K-1 pinned: s = pinned_regime[b] for particle (b, K-1) in place of its inverse-CDF draw
 * (the reference path's regime in a conditional sweep); every other slot, and everything after the regime is chosen, is K31's,
 * in K31's order.  pinned_regime: int32 [B], must not be regime_out.  A pinned regime outside [0, M) writes regime 0 and NaN
 * to that particle and raises AESMC_FLAG_INDEX_OUT_OF_RANGE, as a stored regime outside it does.  Everything else, the
 * step-0 form, the conventions and the statuses as K31's. */
int aesmc_switching_kalman_conditional_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                            const double *mean_in, const double *cov_in, const int64_t *idx,
                                            const double *uniforms, const int32_t *pinned_regime, const void *y,
                                            int32_t *regime_out, double *mean_out, double *cov_out, double *log_weight,
                                            int32_t *flags, int64_t B, int64_t K, void *stream);

/* K48 — the resampling side of a LOOK-AHEAD conditional sweep in one launch: K32 on the stored system (regime, mean, cov) with
 * log_Pi as its log-prior, and K37 on the first-stage log-weights K32 gives.  The stored system of a look-ahead sweep is
 * EQUALLY weighted, so
 *   log_weight[b,j], cdf[b,j,:]   K32's outputs for particle j (the same chains in the same order), written out
 *   idx[b,k]   = K37's free slots over log_weight[b,:] at u[b,k]                                             k = 0 .. K-2
 *   idx[b,K-1] = K37's pinned slot at u[b,K-1] over s[j] = K35's score of particle j against (regime_next[b], factor[b],
 *                lambda[b]) with a log-weight of exactly 0.0 — NOT log_weight[b,j]: the weights that enter ancestor sampling
 *                are those of the stored system
 *   idx[b,K-1] = K - 1         factor and lambda both NULL (no ancestor sampling; regime_next is not read and may be NULL)
 * Operands as K32's (y, y_dtype, the model, of which m0, s0 and the chain's rows are not read) and K37's (u, regime_next,
 * factor, lambda).  Later steps only: the state is not optional.
 * Bad rows as K37's: a NaN first-stage weight (K32's: a stored regime outside [0, M), which also raises
 * AESMC_FLAG_INDEX_OUT_OF_RANGE; a pivot that is not positive under a regime of positive prior) raises
 * AESMC_FLAG_NAN_LOG_WEIGHT, no finite maximum AESMC_FLAG_DEGENERATE_ROW, and every slot of the row is K; the same among s
 * (also: regime_next[b] outside [0, M), with AESMC_FLAG_INDEX_OUT_OF_RANGE) marks only idx[b,K-1] = K.  log_weight and cdf of
 * such particles are NaN, as K32 writes them.
 * aesmc_switching_masked_lookahead_conditional_ancestor_index: the same under K40's mask (observed uint8 [B,Dy], not NULL).
 * The launch keeps log Pi, the model, the scores, for D above 4 a covariance per lane and two arrays of K in LDS: K above
 * aesmc_switching_lookahead_conditional_max_particles(M, D, Dy) = min(aesmc_switching_conditional_max_particles(D),
 * (20480 - [T + P + 30 + M M + M (P P + 2 P + Q P + 2 Q) + (P == 8 ? 256 T : 0) + 256 M]) / 2), with P, Q the extents D, Dy
 * padded to 2, 4 or 8 and T = P (P + 1) / 2 (0 outside the limits of K31), returns AESMC_ERR_UNSUPPORTED, as M, D, Dy above
 * the limits and B K beyond 32-bit element arithmetic do: such a step is composed from K32 and K37.  NULL (but flags; factor
 * and lambda together, and regime_next without them) or misaligned pointers, negative sizes, extents below 1 and an output
 * that is another operand return AESMC_ERR_INVALID_ARGUMENT; B K == 0 is a no-op.  Every check runs before any launch. */
int64_t aesmc_switching_lookahead_conditional_max_particles(int64_t M, int64_t D, int64_t Dy);
int aesmc_switching_lookahead_conditional_ancestor_index(int y_dtype, const aesmc_switching_model *model, const double *log_Pi,
                                                         const int32_t *regime, const double *mean, const double *cov,
                                                         const void *y, const double *u, const int32_t *regime_next,
                                                         const double *factor, const double *lambda, int64_t *out_idx,
                                                         double *log_weight, double *cdf, int32_t *flags, int64_t B,
                                                         int64_t K, void *stream);
int aesmc_switching_masked_lookahead_conditional_ancestor_index(int y_dtype, const aesmc_switching_model *model,
                                                                const double *log_Pi, const int32_t *regime,
                                                                const double *mean, const double *cov, const void *y,
                                                                const uint8_t *observed, const double *u,
                                                                const int32_t *regime_next, const double *factor,
                                                                const double *lambda, int64_t *out_idx, double *log_weight,
                                                                double *cdf, int32_t *flags, int64_t B, int64_t K,
                                                                void *stream);

/* K49 — K31 with K33's and K38's operands at once, the step of a look-ahead conditional sweep: every slot reads its regime from
 * the ancestor's row of particle_cdf [B,K,M] (K48's, K32's), and slot K-1 takes pinned_regime[b] in its place.  The same kernel;
 * checks, conventions and statuses are K33's and K38's together.  Under a mask: aesmc_switching_kalman_masked_step with both. */
int aesmc_switching_kalman_conditional_draw(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                            const double *mean_in, const double *cov_in, const int64_t *idx,
                                            const double *uniforms, const double *particle_cdf, const int32_t *pinned_regime,
                                            const void *y, int32_t *regime_out, double *mean_out, double *cov_out,
                                            double *log_weight, int32_t *flags, int64_t B, int64_t K, void *stream);

/* K39, K40, K41 — K31 (with its K33 and K38 forms), K32 and K34 under a mask of the observation's components.
 *   observed: uint8 [B,Dy], nonzero = component i of y[b] was observed (the storage of a contiguous bool tensor).
 * For batch row b the step is its sibling's on the model with that row's unobserved components deleted from C, d, r and y:
 *   K39, K40   e_i = o_i ? e_i : 0,  U_i. = o_i ? U_i. : 0,  S_ij = (o_i and o_j) ? S_ij : (i == j ? 1 : 0)  — selections of the
 *              sibling's chains, after which everything is the sibling's code: a deleted pivot is 1, its reciprocal 1, its
 *              logarithm 0 (what a padded component's is), and the chains of the kept components gain only products with zeros
 *   K41        e_i = o_i ? y_i - d_i : 0,  1 / r_i^2 -> o_i ? 1 / r_i^2 : 0,  log r_i^2 dropped where o_i is 0
 *   constant   n_b = sum_i o[b,i] in place of Dy
 * With nothing observed K39 is the prediction (log_weight 0, m = m-, P = P-), K40 gives log_weight = logsumexp of the
 * log-priors' row and its cumulative row, K41 only the transition's part.  y at an unobserved position is never used in a
 * chain: it may be NaN or Inf.
 * aesmc_switching_kalman_masked_step: particle_cdf non-NULL is K33's form, pinned_regime non-NULL K38's, both NULL K31's.
 * Checks, conventions and statuses are the siblings'; besides, observed is not NULL and is none of the outputs
 * (AESMC_ERR_INVALID_ARGUMENT).  Every check runs before any launch. */
int aesmc_switching_kalman_masked_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_in,
                                       const double *mean_in, const double *cov_in, const int64_t *idx,
                                       const double *uniforms, const double *particle_cdf, const int32_t *pinned_regime,
                                       const void *y, const uint8_t *observed, int32_t *regime_out, double *mean_out,
                                       double *cov_out, double *log_weight, int32_t *flags, int64_t B, int64_t K,
                                       void *stream);
int aesmc_switching_masked_lookahead(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                                     const int32_t *regime_in, const double *mean_in, const double *cov_in, const void *y,
                                     const uint8_t *observed, double *log_weight, double *cdf, int32_t *flags, int64_t B,
                                     int64_t K, void *stream);
int aesmc_switching_masked_information_step(int y_dtype, const aesmc_switching_model *model, const int32_t *regime_next,
                                            const double *omega_in, const double *lambda_in, const double *c_in,
                                            const void *y, const uint8_t *observed, double *omega_out, double *lambda_out,
                                            double *c_out, double *factor_out, int32_t *flags, int64_t B, int64_t N,
                                            void *stream);

/* K42 — K36 under a mask of the observation of time t+1.  K36 reads no observation, but its cross-covariance adds the
 * information of y_{t+1}, C^T R^-1 C, to Om_{t+1}: under the mask only the observed components add theirs,
 *   Oh = Om_{t+1} + sum_i (o_i ? 1 / r_j[i]^2 : 0) C_j[i,:]^T C_j[i,:],      o = observed_next[b,:] (uint8 [B,Dy], time t+1)
 * — K41's rule; the smoothed mean and covariance do not depend on it.  cross_out and observed_next are not optional here
 * (without a cross-covariance the mask is not read: that is K36 itself), and observed_next is none of the outputs
 * (AESMC_ERR_INVALID_ARGUMENT); everything else, the checks and statuses as K36's. */
int aesmc_switching_masked_smooth_combine(const aesmc_switching_model *model, const int32_t *regime_next, const double *mean,
                                          const double *cov, const double *factor, const double *lambda,
                                          const double *omega_next, const double *cov_next, const uint8_t *observed_next,
                                          double *mean_out, double *cov_out, double *cross_out, int32_t *flags, int64_t B,
                                          int64_t N, int64_t D, void *stream);

/* K43 — K32's scores themselves, for the discrete particle filter of the same model (Fearnhead & Clifford 2003): K32's kernel
 * body as a further instantiation, which writes
 *   scores[b,k,j]   = g_j exactly as K32 defines it: -inf where the log-prior is -inf, NaN where the log-prior is finite and a
 *                     pivot is not positive (and NaN for every j where the stored regime is outside [0, M))
 *   log_weight[b,k] = K32's, bit for bit (the same chains in the same order)
 * and no cumulative row.  scores float64 [B,K,M] takes the place of K32's cdf in every check; the masked form is K40's body
 * in the same way.  Conventions, flags and statuses are K32's (K40's). */
int aesmc_switching_lookahead_scores(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                                     const int32_t *regime_in, const double *mean_in, const double *cov_in, const void *y,
                                     double *scores, double *log_weight, int32_t *flags, int64_t B, int64_t K, void *stream);
int aesmc_switching_masked_lookahead_scores(int y_dtype, const aesmc_switching_model *model, const double *log_prior,
                                            const int32_t *regime_in, const double *mean_in, const double *cov_in,
                                            const void *y, const uint8_t *observed, double *scores, double *log_weight,
                                            int32_t *flags, int64_t B, int64_t K, void *stream);

/* K44 — optimal resampling (Fearnhead & Clifford 2003) of the K_in M candidates of a batch row down to K_out slots, in float64,
 * one launch.  Candidate i = k M + j (particle k, successor regime j):
 *   log_w   float64 [B,K_in] or NULL (zeros)     scores  float64 [B,K_in,M] (K43's)     u  float64 [B] in [0, 1)
 *   a_i     = log_w[b,k] + scores[b,k,j]  (one rounded addition);  top = max_i a_i
 *   e_i     = exp(a_i - top), and 0 where a_i - top < log(2^-1022) (a result below the normal range is flushed: whether a
 *             candidate lives does not hang on how an exponential rounds a subnormal);  live: e_i > 0;  E = sum_i e_i
 *   lse[b]  = top + log E  (the step's evidence increment; the outgoing weights are normalised: no - log K_out)
 * With at most K_out live candidates the survivors are the live candidates in ascending i, log_weight = a_i - lse; the
 * remaining slots are dead: log_weight -inf, parent and regime copies of slot 0's (a valid state of weight zero); count[b] is
 * the number of live candidates.  Otherwise, with w_i = e_i / E:
 *   c       solves sum_i min(1, w_i / c) = K_out: with the candidates by descending weight, L is the smallest number for which
 *           e_(L+1) (K_out - L) < S_L, S_L the sum of e over all but the L heaviest; L is at most K_out - 1 (where the test
 *           fails even there — the mass outside the K_out - 1 heaviest does not register next to the next one — L is
 *           K_out - 1; equal weights are then kept in ascending i); c E = S_L / (K_out - L)
 *   kept    the L heaviest, in ascending i, in slots 0 .. L-1 with log_weight = a_i - lse
 *   thinned with R = K_out - L, Q_i the inclusive running sum of e over the candidates not kept in ascending i and
 *           t_i = R (Q_i / Q_last): slot L + n, n = 0 .. R-1, takes the first candidate not kept with t_i > n + u (n + u
 *           rounded once; the last live one where none is), log_weight = (top + log(Q_last / R)) - lse.  A candidate of
 *           weight 0 is never taken; no candidate is taken twice
 *   parent int64 [B,K_out] (k; `infer`'s ancestor convention), regime int32 [B,K_out] (j), log_weight float64 [B,K_out],
 *   lse float64 [B], count int32 [B] (K_out here)
 * The sums may be added in any order: two evaluations differ only where a w_i lies within rounding of c or an n + u within
 * rounding of a t_i.  A NaN candidate raises AESMC_FLAG_NAN_LOG_WEIGHT, a maximum that is not finite
 * AESMC_FLAG_DEGENERATE_ROW: every parent of the row is K_in (K2's out-of-range marker), every regime 0, log_weight and lse
 * NaN, count 0.  The row's candidates live in LDS: K_in M above aesmc_switching_optimal_resample_max_candidates() (16384), M
 * above the limit of K31 or B K_out beyond 32-bit element arithmetic return AESMC_ERR_UNSUPPORTED.  NULL (but log_w, flags) or
 * misaligned pointers, negative sizes, M below 1 and an output that is an input, another output or flags return
 * AESMC_ERR_INVALID_ARGUMENT; B == 0, K_in == 0 or K_out == 0 is a no-op.  No workspace.  Every check runs before any launch. */
int64_t aesmc_switching_optimal_resample_max_candidates(void);
int aesmc_switching_optimal_resample(const double *log_w, const double *scores, const double *u, int64_t *out_parent,
                                     int32_t *out_regime, double *out_log_weight, double *out_lse, int32_t *out_count,
                                     int32_t *flags, int64_t B, int64_t K_in, int64_t M, int64_t K_out, void *stream);

/* K45, K46 — the expected complete-data sufficient statistics of a switching linear-Gaussian model from per-trajectory smoothed
 * moments (K36's): the reduction between an E-step and a closed-form M-step, or the score by Fisher's identity.  One launch
 * adds ONE timestep's contribution, summed over all trajectories (b, n), to per-workgroup partials in `workspace`;
 * the finishing entry adds the partials in a fixed order and writes out float64 [16, F], row j = the regime s_t
 * (rows M .. 15 are zeros).  With x = (z, 1), X = D + 1, o_c = whether component c of y[b] was observed (K45: always 1),
 * the columns are, in this order (F is what the columns getter returns; packed: element (i, l), i >= l, at i (i + 1) / 2 + l,
 * the constant's index D):
 *   emission block, every t      gram       E[x_t x_t^T] packed                          X (X + 1) / 2
 *                                obs_obs    o_c y_c^2                                     Dy
 *                                obs_state  o_c y_c E[x_t]^T, [c][l]                      Dy X
 *                                grams      K46 only: o_c E[x_t x_t^T] packed, c = 0 ..    Dy X (X + 1) / 2
 *   transition block, t >= 1     counts     1[s_{t-1} = i], i = 0 .. 15                   16
 *                                next_next  E[z_t z_t^T] packed                           D (D + 1) / 2
 *                                next_prev  E[z_t x_{t-1}^T] = [cross + m m'^T, m], [i][l]  D X
 *                                prev_prev  E[x_{t-1} x_{t-1}^T] packed                   X (X + 1) / 2
 *   y float32 / float64 [B,Dy] (y_dtype: AESMC_F32 / AESMC_F64); regime int32 [B,N]; mean [B,N,D], cov [B,N,D(D+1)/2] packed:
 *   the smoothed moments of z_t; regime_prev int32 [B,N], mean_prev, cov_prev (of z_{t-1}) and cross float64 [B,N,D,D]
 *   (cross[i,l] = Cov(z_{t,i}, z_{t-1,l}): rows at the later time) — all four NULL for the t = 0 form, which forms no
 *   transition block, otherwise all four given; observed uint8 [B,Dy] (K46), nonzero = observed.
 *   accumulate 0: the partials are overwritten (the workspace is not read; the t = 0 form writes zeros for the transition
 *   block), 1: added to.  A run of launches that share a workspace must share B, N, D, Dy and the entry.
 * An entry such as P_il + m_i m_l is one float64 fused multiply-add, y_c^2 and y_c m_l one rounded product; the sums are
 * formed on the float64 matrix cores against the indicator of the regime, without floating-point atomics and in one fixed
 * order: the same operands give the same bits.  What must not count is selected to zero before it is summed: the trajectory
 * of a regime or previous regime outside [0, M) contributes nothing and raises AESMC_FLAG_INDEX_OUT_OF_RANGE; in K46, y at
 * an unobserved position is never used and may be NaN or Inf.  A NaN in a moment poisons the sums it enters.
 * The workspace holds the statistics workspace getter's bytes (it depends on D, Dy and the entry only, not on B N).
 * NULL (but flags and the four operands of time t-1) or misaligned pointers, a y_dtype that is neither tag, negative sizes,
 * M, D or Dy below 1, accumulate other than 0 or 1, the four operands of time t-1 given in part, and a workspace that is one of
 * the inputs return AESMC_ERR_INVALID_ARGUMENT; B == 0 or N == 0 is a no-op; D or Dy above 8, M above 16 or B N beyond 32-bit
 * element arithmetic (B N 64 elements) return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch.
 * The finishing entry: `masked` 0 after K45, 1 after K46; B, N, D, Dy those of the launches; out float64 [16, F], not the
 * workspace.  B == 0 or N == 0 is a no-op there too (nothing is written). */
int64_t aesmc_switching_statistics_columns(int64_t D, int64_t Dy, int masked);         /* F; 0 outside the limits */
int64_t aesmc_switching_statistics_workspace_bytes(int64_t D, int64_t Dy, int masked); /* 0 outside the limits */
int aesmc_switching_moment_statistics(int y_dtype, const void *y, const int32_t *regime, const int32_t *regime_prev,
                                      const double *mean_prev, const double *cov_prev, const double *cross,
                                      const double *mean, const double *cov, void *workspace, int accumulate,
                                      int32_t *flags, int64_t B, int64_t N, int64_t M, int64_t D, int64_t Dy, void *stream);
int aesmc_switching_masked_moment_statistics(int y_dtype, const void *y, const uint8_t *observed, const int32_t *regime,
                                             const int32_t *regime_prev, const double *mean_prev, const double *cov_prev,
                                             const double *cross, const double *mean, const double *cov, void *workspace,
                                             int accumulate, int32_t *flags, int64_t B, int64_t N, int64_t M, int64_t D,
                                             int64_t Dy, void *stream);
int aesmc_switching_statistics_finish(const void *workspace, double *out, int masked, int64_t B, int64_t N, int64_t D,
                                      int64_t Dy, void *stream);

/* K47 — the simulation smoother of the continuous state of the same model along GIVEN regime paths (forward filtering,
 * backward sampling; Fruehwirth-Schnatter 1994, Carter & Kohn 1994): z_{0:T-1} ~ p(z | s_{0:T-1}, y) per trajectory, the WHOLE
 * backward pass in one launch.  Trajectory (b,n) has at every time t the conditional Kalman filter's mean m_t and packed
 * covariance P_t (K31 under its regimes — missing observations are already in them: no y and no mask is read) and standard
 * normals eps_t.  One lane per trajectory walks t = T-1 .. 0 with z_{t+1} in registers.  Step T-1 draws from N(m, P) as it
 * stands — unless regime_next and z_next hand over the regime and the drawn state of time T (a long series in chunks; with
 * T = 1 exactly one conditioning step).  A step at t < T-1 (or with them), j = s_{t+1}, q2_i = q_j[i]^2, is a Kalman
 * measurement update with A_j, b_j, diag(q2) as C, d, R and z_{t+1} as y; chains as K34's (float64, every sum ONE chain of
 * fused multiply-adds in ascending index order from the value named first):
 *   V_il = 0 + sum_c A_j[i,c] P_cl;      e_i = (z_{t+1,i} - b_j[i]) - sum_l A_j[i,l] m_l
 *   S_ik = (i == k ? q2_i : 0) + sum_l A_j[i,l] V_kl,  i >= k;      tau = 2^-40 max_i S_ii
 *   L = chol(S) column by column: pivot_k = S_kk - sum_{c<k} L_kc^2; KEPT when pivot_k > tau: rk_k = 1 / sqrt(pivot_k),
 *       L_ik = (S_ik - sum_{c<k} L_ic L_kc) rk_k; otherwise the column is zero and rk_k = 0
 *   v_i  = (e_i - sum_{c<i} L_ic v_c) rk_i;   U_il = (V_il - sum_{c<i} L_ic U_cl) rk_i      (a dropped pivot: a zero row)
 *   P'_ps = P_ps - sum_i U_ip U_is,  p >= s;   m'_p = m_p + sum_i U_ip v_i
 * and then, at every step (at T-1 without z_next: P' = P, m' = m), with tau' = 2^-40 max_i P_ii of the INPUT covariance:
 *   L' = chol(P') by the same rule under tau' (a dropped column is zero);   z_t,p = m'_p + sum_{k<=p} L'_pk eps_t,k.
 * Both matrices are only positive semi-definite — q = 0 components and P = 0 are fine; what a downdate leaves of a direction
 * that z_{t+1} determines is rounding below tau' and is dropped, not taken for variance.
 *   regimes int32 [T,B,N] (regimes[0] is not read);  mean float64 [T,B,N,D];  cov float64 [T,B,N,D(D+1)/2];
 *   noise float64 [T,B,N,D];  regime_next int32 [B,N] and z_next float64 [B,N,D]: both or neither;  states float64 [T,B,N,D]
 * A regime outside [0, M) where it is read (regimes[t], t >= 1, and regime_next) writes NaN to the trajectory's states of
 * every earlier time (t-1 .. 0; T-1 .. 0 for regime_next) and raises AESMC_FLAG_INDEX_OUT_OF_RANGE.  No atomics but the
 * flag's: the same inputs give the same bits.  NULL (but regime_next, z_next, flags) or misaligned pointers, only one of
 * regime_next and z_next, T below 1, negative B or N, M, D or Dy below 1 and states being an input return
 * AESMC_ERR_INVALID_ARGUMENT; B N == 0 is a no-op; D, Dy or M above the limits of K31 or B N D^2 beyond 32-bit element
 * arithmetic return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch.  `flags` may be NULL. */
int aesmc_switching_state_draw(const aesmc_switching_model *model, const int32_t *regimes, const double *mean,
                               const double *cov, const double *noise, const int32_t *regime_next, const double *z_next,
                               double *states, int32_t *flags, int64_t T, int64_t B, int64_t N, void *stream);

/* K50 — the moment-matching collapse of Gaussian mixtures, what the collapsed-mixture filters of the same model (GPB2, which
 * is Kim's filter — Kim 1994; Kim & Nelson 1999 — and IMM, Blom & Bar-Shalom 1988) do between two steps of K31: group (b,g)
 * has N components (lw_n, m_n, P_n) — a log-weight, a mean and a packed covariance — and is replaced by ONE Gaussian with
 * the mixture's mass, mean and covariance.  One lane per group; float64, every sum ONE chain of fused multiply-adds
 * ascending in n from the value named first:
 *   top = max_n lw_n;   e_n = exp(lw_n - top);   sum = 0 + sum_n e_n;   log_mass = top + log(sum);   w_n = e_n (1 / sum)
 *   mean_p = 0 + sum_n w_n m_np
 *   cov_ps = 0 + sum_n [w_n P_n,ps, then (w_n d_np) d_ns],  p >= s,  d_n = m_n - mean      (the centred two-pass form)
 * A group whose every weight is -inf (and one with N == 0) writes log_mass = -inf, a zero mean and a zero covariance.  A
 * component of weight -inf is not read into a chain: its moments may be NaN.  A NaN weight gives NaN outputs for its group.
 *   mean float64 [B,G,N,D] and cov float64 [B,G,N,D(D+1)/2], each with an element stride between groups: the dense one
 *   (N D, N D(D+1)/2), or 0 — the row's N components are shared by its G groups and the operand is [B,N,D], [B,N,D(D+1)/2]
 *   (IMM's mixing: one set of components under M rows of weights);  log_weight float64 [B,G,N];
 *   log_mass float64 [B,G];  mean_out float64 [B,G,D];  cov_out float64 [B,G,D(D+1)/2]
 * No atomics: the same inputs give the same bits.  NULL or misaligned pointers, negative B, G or N, D below 1, a group
 * stride that is neither 0 nor the dense one and an output that is an input or another output return
 * AESMC_ERR_INVALID_ARGUMENT; B G == 0 is a no-op; D above K31's limit, N or G above 256, or B G beyond 32-bit arithmetic
 * return AESMC_ERR_UNSUPPORTED.  Every check runs before any launch. */
int aesmc_switching_collapse(const double *mean, int64_t mean_group_stride, const double *cov, int64_t cov_group_stride,
                             const double *log_weight, double *log_mass, double *mean_out, double *cov_out, int64_t B,
                             int64_t G, int64_t N, int64_t D, void *stream);

/* K51 — a Rauch-Tung-Striebel step between mixture components, the backward step of the collapsed-mixture smoother (Kim
 * 1994): lane (b,i,j) smooths component i filtered at time t, N(m, P), against regime j's smoothed component of time t+1,
 * N(ms, Ps), through A_j, b_j, q2 = q_j^2.  It is K47's measurement update with ms as the observation, and the smoothed
 * covariance carried through the gain; chains and the pivot rule as K47's (float64, every sum ONE chain of fused
 * multiply-adds in ascending index order from the value named first):
 *   V_il = 0 + sum_c A_j[i,c] P_cl;      e_i = (ms_i - b_j[i]) - sum_l A_j[i,l] m_l
 *   S_ik = (i == k ? q2_i : 0) + sum_l A_j[i,l] V_kl,  i >= k;      tau = 2^-40 max_i S_ii
 *   L = chol(S) column by column: pivot_k = S_kk - sum_{c<k} L_kc^2; KEPT when pivot_k > tau: rk_k = 1 / sqrt(pivot_k),
 *       L_ik = (S_ik - sum_{c<k} L_ic L_kc) rk_k; otherwise the column is zero and rk_k = 0
 *   v_i  = (e_i - sum_{c<i} L_ic v_c) rk_i;   U_il = (V_il - sum_{c<i} L_ic U_cl) rk_i;
 *   X_il = (Ps_il - sum_{c<i} L_ic X_cl) rk_i                                              (a dropped pivot: a zero row)
 *   Gm_ik = (X_ik - sum_{c<k} Gm_ic L_kc) rk_k                                             (a dropped pivot: a zero column)
 *   Y_ks = 0 + sum_c Gm_kc U_cs
 *   m'_p = m_p + sum_i U_ip v_i;      P'_ps = P_ps - sum_k U_kp U_ks + sum_k U_kp Y_ks,  p >= s
 * S is only positive semi-definite — q = 0 components and P = 0 are fine (P = 0 returns m and P as they are).
 *   mean float64 [B,M,D] and cov float64 [B,M,D(D+1)/2]: the components filtered at t;  mean_next, cov_next: the same
 *   shapes, smoothed at t+1;  mean_out float64 [B,M,M,D] and cov_out float64 [B,M,M,D(D+1)/2], indexed (b, i, j): i is the
 *   outer index, K50's [B,G,N] layout for the collapse over j that follows.
 * No y, no flags, no atomics: the same inputs give the same bits.  NULL or misaligned pointers, a negative B, M, D or Dy below
 * 1 and an output that is an input or the other output return AESMC_ERR_INVALID_ARGUMENT; B == 0 is a no-op; D, Dy or M
 * above the limits of K31 or B M^2 beyond 32-bit arithmetic return AESMC_ERR_UNSUPPORTED.  Every check runs before any
 * launch. */
int aesmc_switching_pair_smooth(const aesmc_switching_model *model, const double *mean, const double *cov,
                                const double *mean_next, const double *cov_next, double *mean_out, double *cov_out, int64_t B,
                                void *stream);

/* K52 — the adjoint of one step of K31 in the forms the collapsed-mixture filter uses: the regime GIVEN (`regime`, what K31
 * wrote to regime_out: it carries no gradient, so neither the cumulative rows nor the uniforms are read), no ancestors, later
 * steps (mean_in and cov_in given) and step 0 (both NULL: m- = m0, P- = diag(s0^2)).  One lane per slot recomputes the step's
 * forward chains in K31's order (predict, innovation e, U = C P-, S, its factor Lam, v = Lam^-1 e, V = Lam^-1 U) and
 * then, with g = grad_log_weight, mu = grad_mean and G the dense symmetric form of grad_cov (packed covariances: the gradient
 * with respect to a packed element is the derivative of the function of the packed vector, so an off-diagonal element
 * stands for both positions — it enters halved and leaves doubled; what autograd through an unpacking gives):
 *   z = V mu;  alpha = Lam^-T v;  t = Lam^-T z;  ebar = t - g alpha;      Y = v mu^T - 2 V G;  Ubar = Lam^-T Y
 *   Shat = g/2 (v v^T - I) - sym(z v^T) + (V G) V^T;      Sbar = Lam^-T Shat Lam^-1   (triangular solves with the factor; S^-1
 *                                                                                     is never formed)
 *   Hhat = Ubar + Sbar C;      Pbar- = G + sym(C^T Hhat);      mbar- = mu - C^T ebar
 *   grad_C = (Hhat + Sbar C) P- - ebar m-^T;   grad_d = -ebar;   grad_r = 2 r o diag Sbar
 *   later steps:  grad_A = 2 Pbar- (A P) + mbar- m^T;  grad_b = mbar-;  grad_q = 2 q o diag Pbar-;
 *                 grad_mean_in = A^T mbar-;  grad_cov_in = A^T Pbar- A (packed)
 *   step 0:       grad_m0 = mbar-;  grad_s0 = 2 s0 o diag Pbar-
 * (gradients with respect to q, r and s0 themselves, not their squares; y gets none).
 *   regime int32 [B,K];  mean_in float64 [B,K,D], cov_in float64 [B,K,D(D+1)/2] or both NULL;  y [B,Dy] of y_dtype;
 *   grad_mean [B,K,D], grad_cov [B,K,D(D+1)/2], grad_log_weight [B,K] float64: the arriving gradients;
 *   outputs, each of which may be NULL (not wanted, not computed): grad_mean_in [B,K,D], grad_cov_in [B,K,D(D+1)/2] (per
 *   slot; later steps only), grad_m0 [D], grad_s0 [D] (step 0 only), grad_A [M,D,D], grad_b [M,D], grad_q [M,D],
 *   grad_C [M,Dy,D], grad_d [M,Dy], grad_r [M,Dy] (the sums over the slots of each regime; at step 0 the first three are zero).
 * The sums use no floating-point atomics: every slot leaves its row in `workspace`
 * (aesmc_switching_backward_workspace_bytes(B, K, D, Dy) bytes, 8-byte aligned; needed when any of the eight reduced outputs
 * is wanted) and two finishing launches add them per regime and element: the slots are cut into min(64, ceil(B K / 256))
 * consecutive parts; per part, sixteen consecutive runs of slots are added in ascending order and then the sixteen sums in
 * ascending order; then the parts in ascending order.  The same inputs and extents give the same bits.
 * A slot whose three arriving gradients are all exactly zero contributes exactly nothing and writes exact zeros to its rows
 * of the per-slot outputs, even where its recomputed forward is NaN (K31 under an impossible regime).  A regime outside
 * [0, M) raises AESMC_FLAG_INDEX_OUT_OF_RANGE, writes NaN to the slot's per-slot rows and adds nothing to any sum.  A pivot
 * that is not positive gives NaN (per slot and in the sums).
 * NULL model, regime, y or arriving gradients, only one of mean_in and cov_in, all outputs NULL, grad_mean_in or grad_cov_in
 * at step 0, grad_m0 or grad_s0 at a later step, misaligned pointers, negative B or K, M, D or Dy below 1 and an output that
 * is an input or another output return AESMC_ERR_INVALID_ARGUMENT; a reduced output without a workspace, or (non-empty
 * launches) with too small a one, AESMC_ERR_WORKSPACE; B K == 0 is a no-op; D, Dy or M above K31's limits or B K rows beyond
 * 32-bit element arithmetic AESMC_ERR_UNSUPPORTED.  Every check runs before any launch.  `flags` may be NULL. */
int64_t aesmc_switching_backward_workspace_bytes(int64_t B, int64_t K, int64_t D, int64_t Dy);
int aesmc_switching_kalman_step_backward(int y_dtype, const aesmc_switching_model *model, const int32_t *regime,
                                         const double *mean_in, const double *cov_in, const void *y, const double *grad_mean,
                                         const double *grad_cov, const double *grad_log_weight, double *grad_mean_in,
                                         double *grad_cov_in, double *grad_m0, double *grad_s0, double *grad_A, double *grad_b,
                                         double *grad_q, double *grad_C, double *grad_d, double *grad_r, void *workspace,
                                         int64_t workspace_bytes, int32_t *flags, int64_t B, int64_t K, void *stream);

/* K53 — K52 under K39's mask (`observed` uint8 [B,Dy], nonzero = observed; not NULL): the adjoint of
 * aesmc_switching_kalman_masked_step with the regime given.  A deleted component's e, row of U and row and column of S are
 * selected as K39 selects them (its y is never read into a chain and may be NaN), its diagonal entry of Shat is 0, and it
 * contributes exactly nothing to that row's gradients of C, d and r.  Everything else as K52. */
int aesmc_switching_kalman_masked_step_backward(int y_dtype, const aesmc_switching_model *model, const int32_t *regime,
                                                const double *mean_in, const double *cov_in, const void *y,
                                                const uint8_t *observed, const double *grad_mean, const double *grad_cov,
                                                const double *grad_log_weight, double *grad_mean_in, double *grad_cov_in,
                                                double *grad_m0, double *grad_s0, double *grad_A, double *grad_b, double *grad_q,
                                                double *grad_C, double *grad_d, double *grad_r, void *workspace,
                                                int64_t workspace_bytes, int32_t *flags, int64_t B, int64_t K, void *stream);

/* K54 — the adjoint of K50.  K50's inputs (the same layouts and group strides) and the gradients arriving at its outputs,
 * grad_log_mass [B,G], grad_mean_out [B,G,D], grad_cov_out [B,G,D(D+1)/2] (packed, as K52's); with w_n, mean and
 * d_n = m_n - mean recomputed by K50's chains, abar, mu, c the three arriving gradients of the group:
 *   grad_cov_n = w_n c;      grad_mean_n = w_n (mu + 2 sym(c) d_n);      omega_n = <mu, d_n> + <c, P_n + d_n d_n^T>  (packed sums)
 *   grad_log_weight_n = w_n (abar + omega_n - sum_k w_k omega_k)
 * Outputs, each of which may be NULL: grad_log_weight [B,G,N]; grad_mean and grad_cov in the layout of mean and cov — dense
 * [B,G,N,.], or with group stride 0 [B,N,.]: the SUM over the row's G groups, taken in ascending group order inside one
 * lane.  A component of weight -inf is not read and gets gradient exactly zero; a group whose every weight is -inf gives
 * zeros; a NaN weight gives NaN for its group (stride 0: for the row's components).  No atomics: the same inputs give the
 * same bits.  Status codes as K50's; the two strides are both 0 or both dense; all three outputs NULL is
 * AESMC_ERR_INVALID_ARGUMENT. */
int aesmc_switching_collapse_backward(const double *mean, int64_t mean_group_stride, const double *cov, int64_t cov_group_stride,
                                      const double *log_weight, const double *grad_log_mass, const double *grad_mean_out,
                                      const double *grad_cov_out, double *grad_log_weight, double *grad_mean, double *grad_cov,
                                      int64_t B, int64_t G, int64_t N, int64_t D, void *stream);

/* K6— reparameterised Normal draw  out[b,k,j] = loc[b,k,j] + eps[b,k,j] * scale[b,k,j].
 *
 * Replaces the broadcast multiply and the add that follow the noise draw in
 * torch.distributions.Normal.rsample as aesmc/state.py:61-111 (`state.sample`) calls it; the
 * product is rounded before the sum, so the result equals eager PyTorch bit for bit.  `out` is
 * dense [B,K,D]; `eps` (the caller's standard-normal noise), `loc` and `scale` are [B,K,D] views
 * by element strides (0 = broadcast).  eps must be dense in [B,K,D] order or in [K,B,D] order
 * (stride_b = D, stride_k = B*D: the BATCH_EXPANDED draw of aesmc/state.py:102-103, written here
 * directly into [B,K,D] order); other eps layouts return AESMC_ERR_UNSUPPORTED.  `out` must not
 * alias the inputs.
 */
int aesmc_normal_rsample(int dtype, const aesmc_view3 *eps, const aesmc_view3 *loc,
                         const aesmc_view3 *scale, void *out, int64_t B, int64_t K, int64_t D,
                         void *stream);

/* K6 with the noise formed in the launch: out[b,k,j] = loc[b,k,j] + n[b,k,j] * scale[b,k,j], where n is element
 * (b K + k) D + j of the float32 tensor `torch.empty([B,K,D]).normal_()` would hold on this device for a generator at
 * (seed, offset) with ATen's launch geometry `threads` (see aesmc_philox_normal_fill: the same stream, the same
 * Box-Muller, `variant` and `rng_state` as there) — `Normal.rsample` of aesmc/state.py:98 without the noise tensor's
 * round trip through HBM; the caller advances the generator by what `normal_` would have consumed.  float32 only
 * (AESMC_ERR_UNSUPPORTED for float64 and for B K D >= 2^32); `out` is dense [B,K,D], loc and scale [B,K,D] views by
 * element strides (0 = broadcast).  The [K,B,D] noise order of a BATCH_EXPANDED draw is not offered here. */
int aesmc_normal_rsample_drawn(int dtype, const aesmc_view3 *loc, const aesmc_view3 *scale, void *out, int64_t B,
                               int64_t K, int64_t D, uint64_t seed, uint64_t offset, int64_t threads, int variant,
                               const uint64_t *rng_state, void *stream);

/* K7 — weighted particle summaries of a batch row in one pass:
 *   w = softmax_k(log_w[b,:]);  out_mean[b,j] = sum_k w[k] value[b,k,j];
 *   out_second[b,j] = sum_k w[k] value[b,k,j]^2;  out_log_ess[b] = 2 lse(log_w) - lse(2 log_w).
 * Replaces the per-particle Python loop of aesmc/statistics.py:7-76 (empirical_mean; the variance
 * is out_second - out_mean^2 as at statistics.py:75-76) and the two log-sum-exps of
 * aesmc/statistics.py:79-91.  `value` is a [B,K,D] view by element strides (NULL: only the ESS);
 * any of the three outputs may be NULL.  Rows whose weights cannot be normalised (NaN, no finite
 * maximum) give NaN, as the reference's softmax does.  With few batch rows a row is cut into
 * slices of particles, one workgroup each, whose records are merged by a second launch: `ws` must
 * then hold aesmc_particle_summary_workspace_bytes(dtype, B, K, D) bytes (0 = not needed), else
 * AESMC_ERR_WORKSPACE.  Not differentiable: callers that need gradients keep the PyTorch
 * expression.
 */
size_t aesmc_particle_summary_workspace_bytes(int dtype, int64_t B, int64_t K, int64_t D);
int aesmc_particle_summary(int dtype, const void *log_w, const aesmc_view3 *value, void *out_log_ess,
                           void *out_mean, void *out_second, int64_t B, int64_t K, int64_t D, void *ws,
                           size_t ws_bytes, void *stream);

/* ---- linear-Gaussian particle propagation (K8 / K9 / K10) ---------------------------------------
 *
 * An LGSSM written against the reference's callable contract (aesmc/inference.py:20-46) — its own
 * test model included: test/models/lgssm.py:40 (transition, `mult * previous_latents[-1]`), :52
 * (emission) and :66-77 (proposal, a Linear layer of [x_{t-1}, y_t]) — builds every step's
 * distributions as Normal(loc = W x + c, scale) with x the [B,K,d] particles.  `aesmc_affine_map`
 * describes one such location without materialising it:
 *     loc[b,k,j] = offset[b, j] + sum_i weight[j, i] * x[b,k,i]         (dout, din <= aesmc_affine_max_dim())
 * evaluated as ONE chain of fused multiply-adds per element, i ascending, starting from the offset
 * (zero when offset == NULL) — the same chain in all three entry points below, so they agree bit for
 * bit with each other (oracle/smc_core.c restates it with fma()).
 */
typedef struct aesmc_affine_map {
  const void *weight;       /* [dout, din] by element strides; a transposed view is swapped strides */
  int64_t stride_out, stride_in;
  const void *offset;       /* NULL, or offset[b * offset_stride_b + j]: [dout] (stride 0) or [B, dout] */
  int64_t offset_stride_b;
  int64_t dout, din;
} aesmc_affine_map;

int64_t aesmc_affine_max_dim(void); /* 16: larger maps are proper GEMMs and stay library calls */

/* K8 — materialise an affine location (or apply its adjoint):
 *   out[b,k,:] = base[b,k,:] + (offset + W1 x1[b,k,:] + W2 x2[b,k,:])      x2 / m2 and base optional
 * x1 [B,K,m1->din], x2 [B,K,m2->din], base and out [B,K,dout] dense and 16-byte aligned; m2 carries a
 * weight only (its offset is ignored) and m2->dout == m1->dout.  The chain runs through W1's terms,
 * then W2's; base is added last.  Replaces the `[B*K, d] x [d, d]` matmul (+ broadcast add) of the
 * model callables named above, and — with transposed weight views — the input-gradient matmuls of
 * their autograd.  out may alias base. */
int aesmc_particle_affine(int dtype, const void *x1, const aesmc_affine_map *m1, const void *x2,
                          const aesmc_affine_map *m2, const void *base, void *out, int64_t B, int64_t K,
                          void *stream);
/* ... and tanh(location) from the same launch (0.5.0): the device library's tanh — the one torch.tanh calls — applied to the
 * bits the plain launch would store; `tanh(A x_{t-1})` of a nonlinear transition without an element-wise launch behind K8. */
int aesmc_particle_affine_tanh(int dtype, const void *x1, const aesmc_affine_map *m1, const void *x2,
                          const aesmc_affine_map *m2, const void *base, void *out, int64_t B, int64_t K,
                          void *stream);

/* K9 — reparameterised draw from Normal(offset + W source, scale) without the location in HBM:
 *   out[b,k,j] = loc[b,k,j] + eps[b,k,j] * scale          (product rounded before the sum, as K6)
 * `scale` points to ONE value on the device; source [B,K,din], eps and out [B,K,dout] dense, 16-byte
 * aligned, out distinct from both inputs.  Replaces the proposal's matmul + `state.sample`
 * (aesmc/state.py:61-111) for t > 0; equals K8 followed by K6 bit for bit. */
int aesmc_affine_normal_rsample(int dtype, const void *source, const aesmc_affine_map *map, const void *eps,
                                const void *scale, void *out, int64_t B, int64_t K, void *stream);

/* K10 — one SMC step's log-weight (aesmc/inference.py:112-126) for a linear-Gaussian model:
 *   lw[b,k] = sum_j log N(x[b,k,j];  transition(x_prev[b,k,:])_j, scale_p)
 *           + sum_j log N(y[b,j];    emission(x[b,k,:])_j,        scale_g)
 *           - sum_j log N(x[b,k,j];  proposal(x_prev[b,k,:])_j,   scale_q)
 * x_prev, x [B,K,dx] dense and 16-byte aligned; y[b * y_stride_b + j], j < dy = emission->dout (the
 * observation, one row per batch element, not expanded over particles); the three scales point to ONE
 * device value each.  transition and proposal map dx -> dx, emission dx -> dy.  Replaces the three
 * matmuls of the callables and the three `state.log_prob` calls (aesmc/state.py:114-155) + combine.
 * Arithmetic: the three locations by the chain above; per term  q = sum_j (v_j - loc_j)^2  as one fma
 * chain from 0 (j ascending) and  log N = (-q) / (2 scale^2) - d (log scale + log sqrt(2 pi))  —
 * torch.distributions.Normal.log_prob summed over j with the common factors taken out (one division per
 * term instead of one per element); the terms combine as (p + g) - q.  Agrees with K8 x 3 followed by K5
 * to rounding (float64: ~1e-15 relative). */
int aesmc_affine_normal_logweight(int dtype, const void *x_prev, const void *x, const void *y,
                                  int64_t y_stride_b, const aesmc_affine_map *transition,
                                  const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
                                  const void *scale_p, const void *scale_g, const void *scale_q, void *out_lw,
                                  int64_t B, int64_t K, void *stream);

/* K15 — K9 and K10 in one pass: the proposal's reparameterised draw and the step's log-weight together,
 *   out_x[b,k,:] = loc_q(x_prev[b,k,:]) + eps[b,k,:] * scale_q         (K9's arithmetic, the same bits)
 *   out_lw[b,k]  = K10's log-weight of (x_prev, out_x, y)              (the same bits as K10 on out_x)
 * from one read of x_prev and of the noise `eps` [B,K,dx] (dense, 16-byte aligned; out_x likewise and
 * distinct from x_prev; it MAY be the noise's own buffer).  For a model whose transition, emission and
 * proposal are all affine Normals nothing between aesmc/inference.py:106 (`state.sample(proposal)`) and
 * :125-126 (the log-weight) needs x_t's VALUES — the callables only describe distributions in terms of
 * it — so the draw can wait for the launch that weighs it: 520 MB per step at B=1024 K=4096 d=10
 * instead of K9's 503 + K10's 352. */
int aesmc_affine_normal_propagate(int dtype, const void *x_prev, const void *eps, const void *y, int64_t y_stride_b,
                                  const aesmc_affine_map *transition, const aesmc_affine_map *emission,
                                  const aesmc_affine_map *proposal, const void *scale_p, const void *scale_g,
                                  const void *scale_q, void *out_x, void *out_lw, int64_t B, int64_t K, void *stream);

/* K15 through the ancestor indices — the resampling gather folded into the propagation:
 *   x_prev[b,k,:] = x_src[b, ancestors[b,k], :]      (aesmc/inference.py:102-111, state.py:179 `torch.gather`)
 * is formed while the tile is staged and never written: K15 of that x_prev, the same bits as
 * aesmc_resample_gather followed by aesmc_affine_normal_propagate.  `x_src` [B,K,dx] dense and 16-byte
 * aligned, `ancestors` int64 [B,K] (what aesmc_ancestor_index / aesmc_resample_step wrote); an index outside
 * [0, K) is clamped and raises AESMC_FLAG_INDEX_OUT_OF_RANGE in `flags` (may be NULL).  One read of the
 * surviving rows of x_src and of the noise, one write of x_t: 8 dx + 4 dx + 12 B per particle instead of the
 * gather's 8 dx + 8 plus K15's 12 dx + 4.  AESMC_ERR_UNSUPPORTED (caller: gather, then K15) with fewer than
 * ~43 particles per batch row or B K >= 2^31. */
int aesmc_affine_normal_propagate_resampled(
    int dtype, const void *x_src, const int64_t *ancestors, const void *eps, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, void *out_x, void *out_lw, int32_t *flags,
    int64_t B, int64_t K, void *stream);

/* K16 — K15 through the ancestor indices with the noise drawn INSIDE the launch:
 *   eps = the float32 tensor `torch.empty([B,K,dx]).normal_()` holds for a generator at (seed, offset) — see
 *         aesmc_philox_normal_fill below: ATen's launch geometry `threads`, rocRAND's Philox4x32-10 + Box-Muller
 *   x_prev[b,k,:] = x_src[b, ancestors[b,k], :]        (ancestors NULL: x_prev = x_src)
 *   out_x, out_lw = aesmc_affine_normal_propagate(x_prev, eps, ...)        — the same bits
 * Replaces, for one SMC step of a linear-Gaussian model, aesmc/inference.py:102-126: `state.resample` of the
 * newest latent (state.py:179), `state.sample(proposal)` (state.py:98: `_standard_normal`, loc + eps * scale)
 * and the three `state.log_prob` calls.  Neither the noise nor the resampled latent nor any location touches
 * HBM: 8 + 4 dx bytes in, 4 dx + 4 out per particle.  The caller advances the generator by
 * 4 * ceil(B K dx / (4 threads)), as `normal_` would.  float32 only (PyTorch draws float64 noise by another
 * route).  `rng_state` (NULL outside a hipGraph): two uint64 in DEVICE memory, (seed, offset), read by the kernel
 * when it runs — a captured launch replays with whatever generator state the host uploaded before the replay;
 * `seed` is then ignored and `offset` is relative to it (what the captured region had consumed before this
 * launch).  AESMC_ERR_UNSUPPORTED (caller: aesmc_philox_normal_fill, then the launches above) with fewer than
 * 128 particles per batch row (64 below 2^20 particles), dx = 1, or B K dx >= 2^32. */
int aesmc_affine_normal_propagate_drawn(
    const void *x_src, const int64_t *ancestors, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, void *out_x, void *out_lw, int32_t *flags,
    int64_t B, int64_t K, uint64_t seed, uint64_t offset, int64_t threads, const uint64_t *rng_state, void *stream);

/* The same launch with the three maps' weights also at hand as interleaved pairs — `weight_pairs`:
 * aesmc_affine_weight_pairs_floats() float32 values written by aesmc_affine_weight_pairs for the SAME three maps
 * (their values at the time this launch runs: rebuild after the weights change — once per ELBO evaluation, and inside
 * every hipGraph capture) — so that the location chains of two outputs advance together, one v_pk_fma_f32 per input
 * (each half the fused multiply-add of the scalar chain, same order: the same bits, half the multiply-add
 * instructions), and so that weights of any strides (a transposed view) take this form.  NULL: as
 * aesmc_affine_normal_propagate_drawn.  Reference: aesmc/inference.py:102-126 as above. */
int aesmc_affine_normal_propagate_drawn_paired(
    const void *x_src, const int64_t *ancestors, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, void *out_x, void *out_lw, int32_t *flags,
    int64_t B, int64_t K, uint64_t seed, uint64_t offset, int64_t threads, const uint64_t *rng_state,
    const void *weight_pairs, void *stream);

/* aesmc_affine_normal_propagate_drawn_paired reading the ancestors out of the packed words of
 * aesmc_resample_step_packed: x_prev[b,k,:] = x_src[b, ancestor_words[b,k] & 0xffff, :] — 4 bytes per particle in place
 * of 8, every output bit the same.  `ancestor_words` uint32 [B,K], not NULL; a low half >= K is clamped and raises
 * AESMC_FLAG_INDEX_OUT_OF_RANGE as there; `weight_pairs` may be NULL.  Only the launch with one work item per workgroup
 * reads the words: AESMC_ERR_UNSUPPORTED (nothing launched; aesmc_unpack_ancestors, then the entry above) where that form
 * does not cover the operands. */
int aesmc_affine_normal_propagate_drawn_packed(
    const void *x_src, const uint32_t *ancestor_words, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, void *out_x, void *out_lw, int32_t *flags,
    int64_t B, int64_t K, uint64_t seed, uint64_t offset, int64_t threads, const uint64_t *rng_state,
    const void *weight_pairs, void *stream);
/* pairs[map][jp][i] = (W[2 jp][i], W[2 jp + 1][i]), zero where a row or column does not exist, for the transition,
 * emission and proposal maps (float32, extents <= 16, any strides), into `out_pairs` (16-byte aligned device memory of
 * aesmc_affine_weight_pairs_floats() floats).  One small launch. */
int64_t aesmc_affine_weight_pairs_floats(void);
int aesmc_affine_weight_pairs(const aesmc_affine_map *transition, const aesmc_affine_map *emission,
                              const aesmc_affine_map *proposal, void *out_pairs, void *stream);
/* (0.5.1) The same launch with the three scales at hand (device pointers, one float32 each, the values
 * aesmc_affine_normal_propagate_drawn_paired will be handed): behind the pairs it also leaves the launch-wide constants
 * of the three Normal densities of aesmc/state.py:98 — 2 s^2 and d (log s + log(2 pi) / 2) for transition, emission,
 * proposal — and a tag naming the extents they were formed for.  The fused launch then reads them as scalars instead of
 * taking three logarithms in every wavefront (5 % of the vector instructions of a kernel that saturates the vector
 * pipe); the log-weights' bits do not change (the same expressions, evaluated once).  Rebuild whenever a weight OR a
 * scale changes; a buffer written by aesmc_affine_weight_pairs carries a cleared tag and the launch forms the constants
 * itself, as before. */
int aesmc_affine_weight_pairs_scaled(const aesmc_affine_map *transition, const aesmc_affine_map *emission,
                                     const aesmc_affine_map *proposal, const void *scale_p, const void *scale_g,
                                     const void *scale_q, void *out_pairs, void *stream);

/* K20 (0.5.1) — the FIRST step of a run whose proposal and prior do not depend on a latent and whose emission is
 * linear-Gaussian in the latent being drawn (aesmc/inference.py:79-98 with the reference's model style,
 * test/models/lgssm.py: `initial()` a Normal, the time-0 proposal Normal(f(y_0), s) BATCH_EXPANDED, the emission
 * Normal(C x_0 + g, s_g)), float32, latent and observation rows of 1 .. 16 values:
 *   out_x[b,k,:] = loc_q[b,:] + eps[k,b,:] * scale_q[b,:]        (state.py:98, :102-103: `rsample((K,))`, transposed)
 *   out_lw[b,k]  = (sum_j log N(out_x; loc_p, scale_p) + sum_j log N(y_b; C out_x + g, scale_g)) - sum_j log N(out_x; loc_q, scale_q)
 * `eps`: the noise in the reference's order, [K, B, dx] contiguous.  The six views are [B, K, d] views whose stride_k is 0
 * (anything constant along the particles: a scalar, a per-column vector, one row per batch element — any mix); the
 * emission map is C [dy, dx] (any strides) with offset g NULL, [dy] or [B, dy].  One launch in place of
 * aesmc_normal_rsample + aesmc_particle_affine + aesmc_normal_logweight, and the bits of those three: the draw's
 * product is rounded before its sum, the location is one fma chain per output (inputs ascending, started from the
 * offset), an element's log-density (-(d d)) / (2 s s) - log s - log(2 pi) / 2, summed over j ascending from zero.
 * AESMC_ERR_UNSUPPORTED (a view that varies along the particles, rows wider than 16): the caller takes the three. */
int aesmc_affine_normal_initial_step(const void *eps, const aesmc_view3 *loc_q, const aesmc_view3 *scale_q,
                                     const aesmc_view3 *loc_p, const aesmc_view3 *scale_p, const aesmc_view3 *y,
                                     const aesmc_affine_map *emission, const aesmc_view3 *scale_g, void *out_x,
                                     void *out_lw, int64_t B, int64_t K, void *stream);

/* K17 + K18 — one SMC step of a linear-Gaussian model whose latent and observation rows hold 128 float32 values
 * (BASELINE.json configs[4]), the three 128 x 128 maps on the fp32 matrix cores:
 *   x_prev[b,k,:] = x_src[b, ancestors[b,k], :]                              (ancestors NULL: x_prev = x_src)
 *   out_x  = (offset_q + Q x_prev) + eps * s_q                               (each location ONE fma chain per element,
 *   out_lw = (log N(out_x; offset_p + A x_prev, s_p) + log N(y; offset_g + C out_x, s_g)) - log N(out_x; loc_q, s_q)
 *                                                                             inputs ascending: out_x has the C oracle's bits)
 * Replaces aesmc/inference.py:102-126 for one timestep: `state.resample` of the newest latent (state.py:179),
 * `state.sample(proposal)` given its noise `eps` [B,K,128] (state.py:98) and the three `state.log_prob` calls
 * (state.py:114-155) — three library GEMMs, their offsets' broadcast adds, the draw and the log-weight kernel before.
 * Weights [128,128] row-major contiguous (what an nn.Linear holds), offsets NULL / [128] / [B,128], scales one value
 * each, K a multiple of 32; `ws`: aesmc_affine_wide_workspace_bytes(B, K) bytes (two sums per particle between the two
 * launches).  `eps` NULL: the noise is formed in the launch — element e of `torch.empty([B,K,128]).normal_()` for the
 * generator at (seed, offset) with ATen's `threads` (rng_state: as for aesmc_affine_normal_propagate_drawn); covered
 * when K is a multiple of 4 * threads / 128 (configs[4]: threads = 524288, K = 16384), else AESMC_ERR_UNSUPPORTED: the
 * caller fills the noise (aesmc_philox_normal_fill) and passes it.  The squared distances are summed per lane and then over a particle's four lanes: equal to the C oracle's
 * single chain to rounding (2e-6 relative in the tests), not bit for bit.  AESMC_ERR_UNSUPPORTED for every other shape
 * (the caller keeps the route through aesmc_normal_rsample / aesmc_normal_logweight). */
int64_t aesmc_affine_wide_dim(void);      /* 128: the extent with the noise in the launch and the backward pieces below */
size_t aesmc_affine_wide_workspace_bytes(int64_t B, int64_t K);      /* ... at that extent */
/* 0.5.0: the same entry point takes ANY latent width dx with aesmc_affine_wide_min_dim() = 17 <= dx <=
 * aesmc_affine_wide_max_dim() = 256 and any observation width 1 <= dy <= 256 (dx != dy allowed: transition and proposal
 * [dx,dx], emission [dy,dx], y [B,dy], x / eps / out_x [B,K,dx]) and any K — aesmc/state.py:61-183 is dimension-agnostic
 * (rows of at most 16 values are the item kernels': aesmc_affine_normal_propagate_drawn).  Rows are padded to the next of
 * 32 / 48 / 64 / 96 / 128 / 192 / 256 inside the launch (zero inputs leave an fma chain as it is: out_x keeps the C oracle's
 * bits), rows wider than 128 are cut into chunks of output rows (the maps' weights stay LDS-resident per chunk; a
 * particle's partial squared distances meet in `ws`, added in ascending chunk order, for dy > 128 by a third small
 * launch), a batch row's last tile is masked when K is not a multiple of 32, and widths that are not multiples of 4 (rows
 * that are not whole 16-byte pieces) move their pieces of four element by element.  `eps` must be given at these shapes
 * (NULL: AESMC_ERR_UNSUPPORTED — the caller fills the noise with aesmc_philox_normal_fill); `ws`:
 * aesmc_affine_wide_workspace_bytes_for(B, K, dx, dy) bytes. */
int64_t aesmc_affine_wide_min_dim(void);  /* 17 */
int64_t aesmc_affine_wide_max_dim(void);  /* 256 */
size_t aesmc_affine_wide_workspace_bytes_for(int64_t B, int64_t K, int64_t dx, int64_t dy);
int aesmc_affine_normal_propagate_wide(
    const void *x_src, const int64_t *ancestors, const void *eps, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, void *out_x, void *out_lw, void *ws, size_t ws_bytes,
    int32_t *flags, int64_t B, int64_t K, uint64_t seed, uint64_t offset, int64_t threads, const uint64_t *rng_state,
    void *stream);

/* The element-wise parts of the WIDE step's backward (rows of aesmc_affine_wide_dim() = 128 float32 values), between the
 * [B K,128] x [128,128] products a binder runs through its GEMM library — autograd of aesmc/state.py:114-155 (`log_prob` of
 * the emission and the transition) and :98 (the reparameterised draw) for one timestep, recomputed from x_{t-1}, the
 * ancestors, x_t and the log-weights:
 *   aesmc_wide_adjoint_scale: `u` [B,K,128] holds a residual d = value - location (a product's epilogue) — or, with
 *     `base` [B,128] (row stride base_stride_b, a multiple of 4) given, the LOCATION itself, and d = base[b] - u (base = the
 *     value's row minus the map's offset: no [B,K,128] copy of a broadcast row for a product's epilogue to start from); in place
 *     u <- weight[b,k] d / scale^2  (the location's adjoint; weight = the gradient arriving at the particle's log-weight),
 *     out_sq[b,k] = sum_j d_j^2  (the scale's gradient is weight (out_sq / scale^3 - 128 / scale) summed),
 *     out_rows[b, tile, :] = the new u summed over a tile of aesmc_wide_adjoint_tile() = 256 particles (the offset's
 *     gradient is their sum over a row's K / 256 tiles).  out_sq / out_rows may be NULL.
 *   aesmc_wide_adjoint_merge: the same for the transition's residual in `u_p` (or, `value` [B,K,128] given, its LOCATION:
 *     d = (value - base[b]) - u_p, base NULL or as above), and the gradient arriving at x_t in `at_x` takes the term the
 *     transition's density contributes: at_x <- (add + at_x) - u_p (`add` [B,K,128]: what later steps sent to x_t, or NULL);
 *     out_rows_x holds the tiles' sums of the new at_x (the
 *     proposal's offset: the draw carries what arrives at x_t to it).
 * One read and one write per tensor where the PyTorch operations they replace made eight passes and three copies.  float32,
 * dense, 16-byte aligned, K a multiple of 256 (else AESMC_ERR_UNSUPPORTED: the caller keeps its own operations). */
int64_t aesmc_wide_adjoint_tile(void);      /* 256 */
int aesmc_wide_adjoint_scale(void *u, const void *weight, const void *scale, const void *base, int64_t base_stride_b,
                             void *out_sq, void *out_rows, int64_t B, int64_t K, void *stream);
int aesmc_wide_adjoint_merge(void *u_p, void *at_x, const void *weight, const void *scale, const void *value,
                             const void *base, int64_t base_stride_b, const void *add, void *out_sq, void *out_rows_p,
                             void *out_rows_x, int64_t B, int64_t K, void *stream);

/* K13 — a learned proposal net over the particles: the two-layer tanh MLP
 *   out[b,k,:] = layer2->offset + W2 tanh( layer1->offset[b,:] + W1 x[b,k,:] )
 * with W1 [H, din] (din <= 16, H <= aesmc_particle_mlp_max_hidden() = 64), W2 [dout, H] (dout <= 16);
 * layer1->offset is [H] or [B, H] (the per-row part of the first layer: its bias and the observation's
 * columns of the weight applied to y_t), layer2->offset [dout] or NULL.  x, out dense and 16-byte
 * aligned.  Replaces, in a model whose proposal is such a net of [x_{t-1}, y_t] (BASELINE.json configs[3]'s
 * nonlinear state-space model; the reference's own proposal at test/models/lgssm.py:66-77 is its
 * one-layer case), torch.cat + Linear + tanh + Linear: two GEMMs with [B,K,H] round trips through HBM.
 * Returns AESMC_ERR_UNSUPPORTED (caller keeps the PyTorch expression) beyond those extents or with
 * fewer than ~43 particles per batch row.
 * K13b — its backward, recomputing the hidden layer (nothing of [B,K,H] is stored): for grad_out [B,K,dout]
 *   grad_x[b,k,:] = W1^T dh,  dh = (W2^T grad_out) (1 - h^2)                     (dense [B,K,din]; may be NULL)
 *   rec_w1 / rec_w2: [aesmc_particle_mlp_backward_records(B, K)][ceil(H / 16)][256] — per wavefront of the launch the
 *     16 x 16 partials of grad_W1 (rows: 16 hidden units of the chunk, columns: inputs) and grad_W2 (rows: outputs,
 *     columns: the chunk's hidden units), contracted over the particles on the matrix cores; the binder adds the records
 *     (a fixed order: reproducible) and cuts them to [H, din] / [dout, H];
 *   rows: [B K / 256][4][16 ceil(H / 16)] — sum of dh over each wavefront's 64 particles (the gradient of a per-row
 *     layer1->offset is their sum over a row's K / 64 groups); may be NULL.
 *   The output bias' gradient is grad_out summed over the particles (the binder's reduction).
 * K a multiple of 256 (a tile of 256 particles inside one batch row) and din <= 15, else AESMC_ERR_UNSUPPORTED. */
int64_t aesmc_particle_mlp_max_hidden(void);
int aesmc_particle_mlp(int dtype, const void *x, const aesmc_affine_map *layer1, const aesmc_affine_map *layer2,
                       void *out, int64_t B, int64_t K, void *stream);
int64_t aesmc_particle_mlp_backward_records(int64_t B, int64_t K);
int aesmc_particle_mlp_backward(int dtype, const void *x, const void *grad_out, const aesmc_affine_map *layer1,
                                const aesmc_affine_map *layer2, void *grad_x, void *rec_w1, void *rec_w2, void *rows,
                                int64_t B, int64_t K, void *stream);

/* K11 — the adjoint of an affine location  loc = offset + W x  for an incoming gradient grad [B,K,dout]:
 *   out_grad_x[b,k,i]      = sum_j grad[b,k,j] W[j,i]                       (dense [B,K,din])
 *   out_grad_weight[j,i]   = sum_{b,k} grad[b,k,j] x[b,k,i]                 (dense [dout,din])
 * either output may be NULL.  The weight gradient is a contraction over the particle index and runs
 * on the matrix cores (f32 / f64 MFMA: exact fused multiply-adds), each workgroup leaving one 16 x 16
 * partial in `ws` (aesmc_affine_backward_workspace_bytes(dtype, B, K) bytes, 16-byte aligned), summed in
 * workgroup order by a second launch: reproducible run to run.
 *   out_grad_offset[b,j]   = sum_k grad[b,k,j]                              (dense [B,dout]; NULL: not wanted)
 * Replaces the input- and weight-gradient matmuls ([B*K,dout] x [dout,din] and [dout,B*K] x [B*K,din]) and
 * the broadcast-add's reduction of the callables' autograd.  AESMC_ERR_UNSUPPORTED when the offset
 * gradient is asked for with fewer than ~43 particles per batch row (the caller sums grad itself). */
size_t aesmc_affine_backward_workspace_bytes(int dtype, int64_t B, int64_t K);
int aesmc_particle_affine_backward(int dtype, const void *grad, const void *x, const aesmc_affine_map *map,
                                   void *out_grad_x, void *out_grad_weight, void *out_grad_offset, void *ws,
                                   size_t ws_bytes, int64_t B, int64_t K, void *stream);

/* K12 — backward of K10 in one pass over x_prev and x.  The incoming gradient of lw[b,k] is
 *   g = grad_lw[b,k]  (NULL = 0)  +  grad_lse[b] * exp(lw[b,k] - lse[b])  (NULL = 0; K1's backward formed
 *   in place: `lw` is what K10 produced, `lse` its row log-sum-exp — aesmc/inference.py:130-132)
 * and every output pointer of `out` may be NULL (not wanted):
 *   grad_x_prev, grad_x [B,K,dx]      gradients of the two latents (dense, 16-byte aligned);
 *   grad_loc_p, grad_loc_q [B,K,dx], grad_loc_g [B,K,dy]
 *                                     the gradients with respect to the three locations, written only
 *                                     when an OFFSET's gradient is wanted (the caller sums over
 *                                     particles; the observation's gradient is -sum_k grad_loc_g);
 *   grad_weight_p, grad_weight_q [dx,dx], grad_weight_g [dy,dx]
 *                                     weight gradients (matrix cores, partials in `ws` summed in
 *                                     workgroup order by a second launch: reproducible);
 *   grad_scales [3]                   d / d(scale_p, scale_g, scale_q);
 *   grad_offset_p, grad_offset_q [B,dx], grad_offset_g [B,dy]
 *                                     the location gradients summed over each batch row's particles —
 *                                     the gradient of a [B, d] offset (a shared [d] offset: sum the
 *                                     rows; the observation: minus grad_offset_g) — per tile in a fixed
 *                                     order, the tiles of a row added up by one more small launch.
 * `ws`: aesmc_affine_backward_workspace_bytes(dtype, B, K) bytes.  Replaces, for one timestep, the autograd
 * chain of aesmc/inference.py:112-132 through the callables' matmuls: K5's backward, three
 * weight-gradient and three input-gradient matmuls and the adds between them. */
typedef struct aesmc_affine_logweight_grads {
  void *grad_x_prev, *grad_x;
  void *grad_loc_p, *grad_loc_g, *grad_loc_q;
  void *grad_weight_p, *grad_weight_g, *grad_weight_q;
  void *grad_scales;
  void *grad_offset_p, *grad_offset_g, *grad_offset_q;
} aesmc_affine_logweight_grads;

int aesmc_affine_normal_logweight_backward(
    int dtype, const void *x_prev, const void *x, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, const void *lw, const void *lse,
    const void *grad_lse, const void *grad_lw, const aesmc_affine_logweight_grads *out, void *ws, size_t ws_bytes,
    int64_t B, int64_t K, void *stream);

/* K14 — the whole backward of one SMC step whose x_t IS the proposal's reparameterised draw
 *   x_t = loc_q(x_{t-1}) + scale_q * eps        (what K9 produced from the same `proposal` map and `x_prev`),
 * i.e. of aesmc/inference.py:106-132 for a linear-Gaussian model: K12 plus the backward of the draw (K11)
 * plus the accumulations autograd puts between them, in one pass.  `grad_x` [B,K,dx] (dense, 16-byte
 * aligned, or NULL) is the gradient arriving at x_t from later timesteps (the next step's resampling
 * gather); g is formed as in K12.  With
 *   w = grad_x + d/dx_t of g * (log p(x_t | x_{t-1}) + log g(y_t | x_t))
 * the draw carries w to the proposal's parameters and to x_{t-1}; the proposal's density itself depends on
 * them only through eps, which the draw holds fixed, so of its terms only -dx log scale_q survives:
 *   grad_x_prev   = A^T u_p + Q^T w                 (u_p: K12's transition location-gradient)
 *   grad_weight_q = sum_{b,k} w (x) x_{t-1},  grad_offset_q[b] = sum_k w,
 *   grad_scales[2] = sum_{b,k} ( g dx / scale_q + w . eps ),   eps = (x_t - loc_q) / scale_q
 * and the transition's and emission's gradients are K12's.  `out->grad_x` and the three `grad_loc_*`
 * must be NULL (x_t gets no gradient of its own: it is not an independent variable here).  Same
 * workspace, same reproducible finishing launch and same AESMC_ERR_UNSUPPORTED shapes as K12. */
int aesmc_affine_step_backward(
    int dtype, const void *x_prev, const void *x, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, const void *lw, const void *lse,
    const void *grad_lse, const void *grad_lw, const void *grad_x, const aesmc_affine_logweight_grads *out,
    void *ws, size_t ws_bytes, int64_t B, int64_t K, void *stream);

/* K14 through the ancestor indices: `x_src` is the UN-resampled x_{t-1} and the step's x_prev its rows
 * x_src[b, ancestors[b,k], :] fetched while the tile is staged (the forward step — aesmc_affine_normal_propagate_
 * resampled / _drawn — never wrote them, neither does the backward).  Everything else as
 * aesmc_affine_step_backward; `out->grad_x_prev` is the gradient with respect to the RESAMPLED rows
 * ([B,K,dx], one per child): the caller sums children into their ancestors (aesmc_resample_gather_backward),
 * which is torch.gather's backward (aesmc/state.py:179).  An ancestor outside [0, K) is clamped and raises
 * AESMC_FLAG_INDEX_OUT_OF_RANGE in `flags` (may be NULL).
 * `child_grad` / `child_end` (both or neither; NULL = none): the gradient that reaches x_t from the NEXT step when
 * that step, too, resampled through ancestors — its `out->grad_x_prev`, one row per CHILD [B,K,dx] — and the next
 * resampling step's children ranges (aesmc_resample_step_ranges).  The kernel then adds, to whatever `grad_x`
 * brings, the sum of each particle's children's rows (a lane adds its own particle's run in k order; what lies beyond
 * the first 32 children of a run — a collapsed particle system — is shared out over the wavefront, in a fixed order):
 * torch.gather's backward without its launch and without the [B,K,dx] round trip of the summed gradient.
 * `chain` (may be NULL): consecutive steps of a time-homogeneous model share A, C, Q and the scales, and autograd only
 * ever wants the SUM of their gradients over the steps (aesmc/inference.py:60-135 calls the same callables every
 * step).  A call with `chain->defer` non-zero leaves its sums as per-workgroup records in `ws` (grad_weight_* and
 * grad_scales of `out` must be NULL; `chain->records` receives their count; defer = 2 where the scales' gradients are
 * wanted in the end, which costs the proposal's location as a non-NULL grad_scales does) instead of finishing them; the next call
 * names that workspace in `chain->carry` / `carry_records` and each of its workgroups starts from the records it is
 * handed (record w, w + grid, ... in that order), so the run of steps is finished once, by its last call — or by
 * aesmc_affine_backward_collect.  The row sums (offset gradients: per step) are finished by every call. */
typedef struct {
  const void *carry;      /* in: workspace of the call whose records this one continues, or NULL */
  int32_t carry_records;  /* in: how many records it holds (what that call left in `records`) */
  int32_t defer;          /* in: non-zero = leave this call's sums as records in `ws` (2: the scales' among them) */
  int32_t records;        /* out: records this call left in `ws` */
  const void *pairs_in;   /* in: the three maps' interleaved weight pairs as an EARLIER call of this run left them in
                           *     `pairs_out` (the same weights: a run shares them), or NULL: this call writes its own into
                           *     its workspace's tail (one small launch in front) */
  void *pairs_out;        /* out: where the pairs this call used lie (its own, or `pairs_in` handed on), NULL if it used
                           *      none; valid while the workspace that holds them is */
} aesmc_affine_chain;
int aesmc_affine_step_backward_resampled(
    int dtype, const void *x_src, const int64_t *ancestors, const void *x, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, const void *lw, const void *lse,
    const void *grad_lse, const void *grad_lw, const void *grad_x, const void *child_grad, const int32_t *child_end,
    const aesmc_affine_logweight_grads *out, void *ws, size_t ws_bytes, int32_t *flags, aesmc_affine_chain *chain,
    int64_t B, int64_t K, void *stream);

/* aesmc_affine_step_backward_resampled with the packed words of aesmc_resample_step_packed in place of the two arrays:
 * `ancestor_words` (uint32 [B,K], not NULL) are the words of the resampling step in front of THIS step — their low
 * halves are its ancestors —, `child_words` (NULL exactly when child_grad is) those of the NEXT step's — their high
 * halves are where each particle's children end.  Every gradient and record equals, bit for bit, what the entry above
 * forms from the unpacked arrays.  float32, rows of an even number (2 .. 14) of values on both sides, K a multiple of 256
 * (the form of the kernel that keeps a wavefront's rows in registers); AESMC_ERR_UNSUPPORTED elsewhere, nothing
 * launched: aesmc_unpack_ancestors, then the entry above. */
int aesmc_affine_step_backward_packed(
    int dtype, const void *x_src, const uint32_t *ancestor_words, const void *x, const void *y, int64_t y_stride_b,
    const aesmc_affine_map *transition, const aesmc_affine_map *emission, const aesmc_affine_map *proposal,
    const void *scale_p, const void *scale_g, const void *scale_q, const void *lw, const void *lse,
    const void *grad_lse, const void *grad_lw, const void *grad_x, const void *child_grad, const uint32_t *child_words,
    const aesmc_affine_logweight_grads *out, void *ws, size_t ws_bytes, int32_t *flags, aesmc_affine_chain *chain,
    int64_t B, int64_t K, void *stream);

/* The finishing launch of K14 alone: grad_weight_p / _g / _q and grad_scales of `out` (each may be NULL) from the
 * `records` records a deferring aesmc_affine_step_backward_resampled call left in `ws` — for a run of steps whose last
 * call could not carry them on. */
int aesmc_affine_backward_collect(int dtype, const void *ws, int32_t records, int64_t dx, int64_t dy,
                                  const aesmc_affine_logweight_grads *out, void *stream);

/* Noise — the float32 tensor `torch.empty(numel).normal_()` holds on this device for a generator at
 * (seed, offset): out[e], e < numel.  Replaces, inside a kernel or on its own, the `_standard_normal` draw of
 * `Normal.rsample` (aesmc/state.py:98; torch/distributions/normal.py rsample) WITHOUT leaving PyTorch's
 * stream: ATen's launch geometry (`threads` = 256 * min(#CU * maxThreadsPerCU / 256, ceil(numel / 256)), the
 * caller computes it from the device properties), rocRAND's Philox4x32-10 and Box-Muller restated
 * (csrc/philox_normal.hpp).  The caller advances the generator by 4 * ceil(numel / (4 * threads)), what
 * `normal_` would have consumed.  offset must be a multiple of 4 (PyTorch's always is).  `variant` 0 is
 * the product (Box-Muller's affine maps as fused multiply-adds, as PyTorch's build of rocRAND has them);
 * 1 = separate multiply and add, kept for the test that shows which of the two PyTorch's build uses.
 * `rng_state`: as for aesmc_affine_normal_propagate_drawn (NULL outside a hipGraph). */
int aesmc_philox_normal_fill(void *out, int64_t numel, uint64_t seed, uint64_t offset, int64_t threads, int variant,
                             const uint64_t *rng_state, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AESMC_HIP_H_ */
