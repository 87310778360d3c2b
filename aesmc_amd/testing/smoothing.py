"""NumPy statement of the CONTRACT of the backward-simulation kernel (include/aesmc_hip.h, aesmc_backward_sample),
written without regard to the kernel's structure (no tiles, no chunks, no passes) — what the tests hold the HIP result to,
exactly — and of the whole backward pass that `aesmc_amd.smoothing.backward_simulate` makes of it.  Below it the same
for the marginal smoother: the pairwise log-sum-exp (aesmc_pairwise_lse), the bound its kernel is held to, and the
backward recursion that `aesmc_amd.smoothing.marginal_log_weights` makes of it; and for the two-slice smoother: the
pairwise softmax mean (aesmc_pairwise_mean), its bound, and the recursion of `aesmc_amd.smoothing.two_slice_expectation`;
and for the MAP trajectory: the pairwise max and argmax (aesmc_pairwise_argmax), its bound, and the Viterbi recursion of
`aesmc_amd.smoothing.map_trajectory`.

One backward step of forward filtering / backward simulation (Godsill, Doucet & West 2004): trajectory m, whose state at
t+1 is target[b,m], draws particle k of step t with probability proportional to

    exp(log_w[b,k]) * Normal(target[b,m]; loc[b,k], scale)

by inverting the running sum of those weights at u[b,m].  (This package never imports the oracle — tests/test_library.py.)
"""
import numpy as np

FLAG_NAN_LOG_WEIGHT = 1
FLAG_DEGENERATE_ROW = 2

# below this the kernels' float64 exp of a non-positive number (csrc/ancestor_index.hpp) is zero
EXP_UNDERFLOW = -745.2


def backward_weights(log_w_row, loc_row, target_row, scale):
    """(w [M,K] float64, nan [M] bool, degenerate [M] bool) of one batch row: log_w_row [K], loc_row [K,D] or None,
    target_row [M,D] or None (then M comes from nowhere: pass a [M,0] array), scale [D] or one value."""
    lw = np.asarray(log_w_row).astype(np.float64)
    K = lw.shape[0]
    target = np.asarray(target_row)
    M, D = target.shape
    q = np.zeros((M, K), dtype=np.float64)
    if D:
        loc = np.asarray(loc_row).astype(np.float64)
        inv = 1.0 / np.broadcast_to(np.asarray(scale).astype(np.float64).reshape(-1), (D,))
        with np.errstate(invalid="ignore", over="ignore"):
            for d in range(D):
                q = q + ((target[:, d].astype(np.float64)[:, None] - loc[None, :, d]) * inv[d]) ** 2
    with np.errstate(invalid="ignore", over="ignore"):
        s = lw[None, :] - 0.5 * q
        nan = np.isnan(s).any(axis=1)
        smax = np.where(nan, 0.0, np.max(np.where(np.isnan(s), -np.inf, s), axis=1))
        degenerate = ~nan & ~np.isfinite(smax)
        x = s - np.where(nan | degenerate, 0.0, smax)[:, None]
        w = np.where(x > EXP_UNDERFLOW, np.exp(np.minimum(x, 0.0)), 0.0)
    return w, nan, degenerate


def backward_sample(log_w, loc, target, scale, u, payload=None):
    """log_w [B,K]; loc [B,K,D] / target [B,M,D] / scale (one value or [D]) or all three None (no transition term);
    u [B,M] float64 in [0, 1); payload [B,K,...] or None -> (idx int64 [B,M], flags, payload[b, idx[b,m]] or None).

        idx[b,m] = min( #{k : C[m,k] <= u[b,m] * C[m,K-1]},  max{k : w[m,k] > 0} ),   C = cumsum(w[m,:])

    A NaN among a trajectory's scores: FLAG_NAN_LOG_WEIGHT and idx = K; no finite maximum: FLAG_DEGENERATE_ROW and idx = K.
    The payload of idx == K is particle K-1's."""
    log_w = np.asarray(log_w)
    B, K = log_w.shape
    u = np.asarray(u, dtype=np.float64)
    M = u.shape[1]
    if u.shape != (B, M):
        raise ValueError("one uniform per trajectory: u must be [{}, M], got {}".format(B, u.shape))
    if loc is None:
        loc3, target3 = np.zeros((B, K, 0)), np.zeros((B, M, 0))
    else:
        loc3, target3 = np.asarray(loc).reshape(B, K, -1), np.asarray(target).reshape(B, M, -1)
    idx = np.empty((B, M), dtype=np.int64)
    flags = 0
    for b in range(B):
        w, nan, degenerate = backward_weights(log_w[b], loc3[b], target3[b], scale)
        if nan.any():
            flags |= FLAG_NAN_LOG_WEIGHT
        if degenerate.any():
            flags |= FLAG_DEGENERATE_ROW
        for m in range(M):
            if nan[m] or degenerate[m]:
                idx[b, m] = K
                continue
            c = np.cumsum(w[m])
            count = int(np.searchsorted(c, u[b, m] * c[-1], side="right"))
            idx[b, m] = min(count, int(np.flatnonzero(w[m] > 0)[-1]))
    moved = None
    if payload is not None:
        payload = np.asarray(payload)
        moved = np.stack([payload[b][np.minimum(idx[b], K - 1)] for b in range(B)])
    return idx, flags, moved


def backward_pass(latents, log_weights, locations, scale, uniforms):
    """The whole backward pass: latents T x [B,K,...], log_weights T x [B,K], locations(t) -> the transition's location
    [B,K,...] of step t's stored particles for time t+1, scale as above, uniforms T x [B,M] (block t draws step t).
    Returns (trajectories T x [B,M,...], indices T x [B,M])."""
    T = len(latents)
    states, indices = [None] * T, [None] * T
    indices[-1], _, states[-1] = backward_sample(log_weights[-1], None, None, None, uniforms[-1], latents[-1])
    for t in range(T - 2, -1, -1):
        indices[t], _, states[t] = backward_sample(log_weights[t], locations(t), states[t + 1], scale, uniforms[t],
                                                   latents[t])
    return states, indices


# ---- the marginal smoother (FFBSm; Huerzeler & Kuensch 1998, Doucet, Godsill & Andrieu 2000) --------------------------------
EPSILON = 2.0 ** -52
NEAR_THE_MAXIMUM = 40.0      # columns further below a row point's maximum carry less than C e^-40 of its sum


def _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add):
    """float64 (rows [B,R,D], cols [B,C,D], inv [D], col_a [B,C], col_sub [B,C] or None, row_add [B,R] or None)."""
    col_a = np.asarray(col_a)
    B, C = col_a.shape
    rows, cols = np.asarray(rows), np.asarray(cols)
    R = rows.shape[1]
    D = int(np.prod(rows.shape[2:], dtype=np.int64))
    wide = lambda a: None if a is None else np.asarray(a).astype(np.float64)
    inv = np.zeros(0)
    if D:
        inv = 1.0 / np.broadcast_to(wide(scale).reshape(-1), (D,))
    return wide(rows).reshape(B, R, D), wide(cols).reshape(B, C, D), inv, wide(col_a), wide(col_sub), wide(row_add)


def _pairwise_scores(rows_b, cols_b, inv, col_a_b, col_sub_b):
    """(s [R,C], term [C], q [R,C]) of one batch row, float64."""
    R, C = rows_b.shape[0], cols_b.shape[0]
    q = np.zeros((R, C), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(rows_b.shape[1]):
            q = q + ((rows_b[:, None, d] - cols_b[None, :, d]) * inv[d]) ** 2
        term = col_a_b if col_sub_b is None else np.where(col_a_b == -np.inf, -np.inf, col_a_b - col_sub_b)
        s = term[None, :] - 0.5 * q
    return s, term, q


def pairwise_lse(rows, cols, scale, col_a, col_sub=None, row_add=None):
    """rows [B,R,...], cols [B,C,...] (trailing dims flattened to D values; none: no distance term), scale one value or
    [D], col_a / col_sub [B,C], row_add [B,R] -> (out float64 [B,R], flags):

        out[b,r] = row_add[b,r] + log sum_c exp( term[b,c] - 1/2 sum_d ((rows[b,r,d] - cols[b,c,d]) / scale[d])^2 )
        term[b,c] = col_a[b,c] - col_sub[b,c],   -inf where col_a[b,c] == -inf whatever col_sub holds

    in float64 whatever the operands' dtype is.  A NaN among a row point's scores or in its row_add: FLAG_NAN_LOG_WEIGHT and
    NaN; else a maximum score of +inf: FLAG_DEGENERATE_ROW and +inf; else every score -inf: -inf and no flag."""
    rows, cols, inv, col_a, col_sub, row_add = _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add)
    B, R = rows.shape[:2]
    out = np.empty((B, R), dtype=np.float64)
    flags = 0
    for b in range(B):
        s, _, _ = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        add = np.zeros(R) if row_add is None else row_add[b]
        nan = np.isnan(s).any(axis=1) | np.isnan(add)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            smax = np.max(np.where(np.isnan(s), -np.inf, s), axis=1)
            finite = np.isfinite(smax) & ~nan
            x = s - np.where(finite, smax, 0.0)[:, None]
            w = np.where(x > EXP_UNDERFLOW, np.exp(np.minimum(x, 0.0)), 0.0)
            value = add + (smax + np.log(w.sum(axis=1)))
        value = np.where(finite, value, smax)          # +inf and -inf as they are, whatever row_add holds
        out[b] = np.where(nan, np.nan, value)
        if nan.any():
            flags |= FLAG_NAN_LOG_WEIGHT
        if (~nan & (smax == np.inf)).any():
            flags |= FLAG_DEGENERATE_ROW
    return out, flags


def pairwise_lse_bound(rows, cols, scale, col_a, col_sub=None, row_add=None):
    """[B,R] float64: how far a float64 evaluation of `pairwise_lse` in another order may lie from this one, derived and
    not measured.  With eps = 2^-52, D values per point and C columns

        bound[b,r] = eps * ( (D + 4) * max_c (|term[b,c]| + q[r,c] / 2)  +  C + 8 )

    the maximum over the columns whose score lies within 40 of the row point's largest: the first part is fused against
    separately rounded multiply-adds (and the order of the D additions) in the scores that matter, the second any order
    of the C additions plus exp and log; columns further down carry less than C e^-40 of the sum.  Zero where the result
    is not finite (those are conventions, held exactly)."""
    rows, cols, inv, col_a, col_sub, row_add = _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add)
    B, R, D = rows.shape
    C = cols.shape[1]
    bound = np.zeros((B, R), dtype=np.float64)
    for b in range(B):
        s, term, q = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        with np.errstate(invalid="ignore"):
            smax = np.max(np.where(np.isnan(s), -np.inf, s), axis=1)
            finite = np.isfinite(smax) & ~np.isnan(s).any(axis=1)
            near = s >= (smax - NEAR_THE_MAXIMUM)[:, None]
            size = np.where(near, np.abs(term)[None, :] + 0.5 * q, 0.0).max(axis=1)
        bound[b] = np.where(finite, EPSILON * ((D + 4) * np.where(finite, size, 0.0) + C + 8), 0.0)
    return bound


def marginal_pass(latents, log_weights, locations, scale, return_tolerance=False):
    """The whole backward recursion of the marginal smoother: latents T x [B,K,...], log_weights T x [B,K], locations(t)
    -> the transition's location [B,K,...] of step t's stored particles for time t+1, scale as above.  Returns T x [B,K]
    smoothed log-weights in log_weights' dtype:

        ls[T-1] = log_w[T-1] - logsumexp(log_w[T-1])
        den[j]  = log sum_l exp(log_w[t][l] - 1/2 |x[t+1][j] - loc[l]|^2)                         (pairwise_lse)
        ls[t]   = log_w[t] + log sum_j exp(ls[t+1][j] - den[j] - 1/2 |loc[i] - x[t+1][j]|^2)      (pairwise_lse)

    (|.|^2 in units of the scale), every pairwise_lse rounded to that dtype as the device's launches round theirs.
    `return_tolerance`: also T x [B,K] float64, how far an evaluation that keeps every launch within `pairwise_lse_bound`
    (and, in float32, within one unit in the last place of the rounding) may lie from this one: log-sum-exp moves by
    at most the largest move of its terms, so a step's tolerance is the largest of the step after it plus the largest of
    its denominators' plus its own; the last step's is four units in the last place of the row's log-sum-exp and of the
    result (the log-sum-exp in the dtype's own arithmetic, one subtraction)."""
    T = len(latents)
    dtype = np.asarray(log_weights[-1]).dtype

    def last_place(v):      # of the rounding to the dtype: float64 results are not rounded again
        if dtype == np.float64:
            return np.zeros(v.shape)
        return np.where(np.isfinite(v), np.spacing(np.abs(np.where(np.isfinite(v), v, 0)).astype(dtype)), 0).astype(np.float64)

    smoothed, tolerance = [None] * T, [None] * T
    log_w = np.asarray(log_weights[-1]).astype(np.float64)
    top = log_w.max(axis=1, keepdims=True)
    lse = top + np.log(np.exp(log_w - top).sum(axis=1, keepdims=True))
    smoothed[-1] = (log_w - lse).astype(dtype)
    tolerance[-1] = 4.0 * float(np.finfo(dtype).eps) * (np.abs(lse) + np.abs(log_w - lse))
    for t in range(T - 2, -1, -1):
        loc, nxt, log_w = locations(t), latents[t + 1], log_weights[t]
        den = pairwise_lse(nxt, loc, scale, log_w)[0].astype(dtype)
        out = pairwise_lse(loc, nxt, scale, smoothed[t + 1], den, log_w)[0].astype(dtype)
        smoothed[t] = out
        den_tolerance = pairwise_lse_bound(nxt, loc, scale, log_w) + last_place(den)
        tolerance[t] = (tolerance[t + 1].max(axis=1, keepdims=True) + den_tolerance.max(axis=1, keepdims=True) +
                        pairwise_lse_bound(loc, nxt, scale, smoothed[t + 1], den, log_w) + last_place(out))
    return (smoothed, tolerance) if return_tolerance else smoothed


# ---- the two-slice smoother: E[g(x_{t+1}) f(x_t)^T | y_0..y_{T-1}] from the same recursion ----------------------------------
def _payload_operand(payload, B, C):
    payload = np.asarray(payload)
    if payload.shape[:2] != (B, C):
        raise ValueError("one payload per column: payload must be [{}, {}, ...], got {}".format(B, C, payload.shape))
    return payload.astype(np.float64).reshape(B, C, -1)


def _softmax_weights(s, add):
    """(w [R,C] = exp(s - smax) with the kernels' underflow, nan [R], smax [R], finite [R]) of one batch row."""
    nan = np.isnan(s).any(axis=1) | np.isnan(add)
    with np.errstate(invalid="ignore", over="ignore"):
        smax = np.max(np.where(np.isnan(s), -np.inf, s), axis=1)
        finite = np.isfinite(smax) & ~nan
        x = s - np.where(finite, smax, 0.0)[:, None]
        w = np.where(x > EXP_UNDERFLOW, np.exp(np.minimum(x, 0.0)), 0.0)
    return np.where(finite[:, None], w, 0.0), nan, smax, finite


def pairwise_mean(rows, cols, scale, col_a, payload, col_sub=None, row_add=None):
    """Operands as `pairwise_lse` takes them, payload [B,C,...] (trailing dims flattened to P values) ->
    (out float64 [B,R,P], lse float64 [B,R], flags):

        s[b,r,c]   = term[b,c] - 1/2 sum_d ((rows[b,r,d] - cols[b,c,d]) / scale[d])^2        (term as pairwise_lse forms it)
        out[b,r,p] = sum_c softmax_c(s[b,r,:])[c] * payload[b,c,p]
        lse[b,r]   = pairwise_lse(rows, cols, scale, col_a, col_sub, row_add)[b,r]

    in float64 whatever the operands' dtype is: sum_c e_c payload_c / sum_c e_c with e_c = exp(s_c - max s), a true
    division.  Conventions, per row point (row points and batch rows never affect one another):
      a column with col_a == -inf is absent: its payload is SELECTED out (replaced by zero, not multiplied by a zero weight),
        so whatever it holds (NaN, inf) never reaches a result.  The payload of a present column must be finite;
      a NaN among the row point's scores or in its row_add: FLAG_NAN_LOG_WEIGHT, its P values and its lse NaN;
      else a largest score of +inf: FLAG_DEGENERATE_ROW, lse +inf and its P values NaN (there are no weights to average with);
      else every score -inf: out 0, lse -inf and no flag — a point of zero weight."""
    lse, flags = pairwise_lse(rows, cols, scale, col_a, col_sub, row_add)
    rows, cols, inv, col_a, col_sub, row_add = _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add)
    B, R = rows.shape[:2]
    C = cols.shape[1]
    payload = _payload_operand(payload, B, C)
    out = np.empty((B, R, payload.shape[2]), dtype=np.float64)
    for b in range(B):
        s, _, _ = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        w, nan, smax, finite = _softmax_weights(s, np.zeros(R) if row_add is None else row_add[b])
        held = np.where((col_a[b] == -np.inf)[:, None], 0.0, payload[b])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mean = (w[:, :, None] * held[None, :, :]).sum(axis=1) / w.sum(axis=1)[:, None]
        mean = np.where((smax == -np.inf)[:, None] & ~nan[:, None], 0.0, np.where(finite[:, None], mean, np.nan))
        out[b] = mean
    return out, lse, flags


def pairwise_mean_bound(rows, cols, scale, col_a, payload, col_sub=None, row_add=None):
    """[B,R,P] float64: how far a float64 evaluation of `pairwise_mean`'s `out` in another order (other tiles, a running
    reference instead of the maximum, fused against separately rounded multiply-adds, matrix cores against the vector
    pipe) may lie from this one, derived and not measured:

        bound[b,r,p] = 2 * pairwise_lse_bound[b,r] * sum_c softmax_c(s[b,r,:])[c] * |payload[b,c,p]|

    out = N / Z with N = sum_c e_c v_c and Z = sum_c e_c.  Let delta = eps * (D + 4) * max_c (|term| + q / 2) bound the
    move of a score that matters, as in `pairwise_lse_bound`: every e_c moves by the factor exp(+-delta) (plus exp's own
    few eps and one for the product with v_c, the `+ 8` there), so N moves by at most delta' * sum_c e_c |v_c| and Z by
    delta' * Z; the C additions of either sum, in any order, move it by at most eps * C times the sum of the magnitudes.
    Both together are pairwise_lse_bound = eps * ((D + 4) * size + C + 8), once for N — relative to sum_c e_c |v_c| — and
    once for Z; divided by Z that is twice the bound times sum_c softmax_c |v_c|, to first order.  The payload enters
    through its magnitude under the row point's own weights, so cancellation in N is covered.  Zero where the result is not
    finite or the payload under the weights is zero (conventions and exact zeros, held exactly)."""
    scores = pairwise_lse_bound(rows, cols, scale, col_a, col_sub, row_add)
    rows, cols, inv, col_a, col_sub, row_add = _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add)
    B, R = rows.shape[:2]
    payload = _payload_operand(payload, B, cols.shape[1])
    bound = np.zeros((B, R, payload.shape[2]), dtype=np.float64)
    for b in range(B):
        s, _, _ = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        w, _, _, finite = _softmax_weights(s, np.zeros(R) if row_add is None else row_add[b])
        held = np.abs(np.where((col_a[b] == -np.inf)[:, None], 0.0, payload[b]))
        with np.errstate(invalid="ignore", divide="ignore"):
            size = (w[:, :, None] * held[None, :, :]).sum(axis=1) / w.sum(axis=1)[:, None]
        bound[b] = np.where(finite[:, None], 2.0 * scores[b][:, None] * np.where(finite[:, None], size, 0.0), 0.0)
    return bound


def two_slice_pass(latents, log_weights, locations, scale, previous=None, following=None, return_tolerance=False):
    """The whole backward recursion of the two-slice smoother: latents, log_weights, locations, scale as `marginal_pass`
    takes them; previous / following: None (the latent itself, trailing dims flattened) or callables (time, latent
    [B,K,...]) -> array [B,K,...], flattened to P and Q values — previous is called with (t, latents[t]), following with
    (t + 1, latents[t + 1]), once per step.  Returns (expectations, smoothed): T-1 arrays [B,Q,P] and T arrays [B,K], in
    log_weights' dtype:

        m[j], den[j] = pairwise_mean(x[t+1], loc, scale, log_w[t], previous(t, x[t]))          (one launch)
        ls[t]        = pairwise_lse(loc, x[t+1], scale, ls[t+1], den, log_w[t])                (one launch: marginal_pass's)
        E[t][q,p]    = sum_j exp(ls[t+1][j]) following(t+1, x[t+1])[j,q] m[j,p]
                     = E[following_q(x_{t+1}) previous_p(x_t) | y_0..y_{T-1}]

    every launch rounded to that dtype as the device's launches round theirs, the contraction in float64 and rounded once.
    `return_tolerance`: also (T-1 x [B,Q,P], T x [B,K]) float64, how far an evaluation that keeps every launch within its
    bound (and, in float32, within one unit in the last place of the rounding) may lie from this one.  The smoothed
    log-weights' is `marginal_pass`'s.  The expectations': m[j,p] moves by pairwise_mean_bound plus its last place, the
    weight exp(ls[t+1][j]) by the factor exp(+-tau_j) with tau the smoothed log-weights' tolerance (to first order tau_j,
    doubled to cover the second), the K additions and the products by eps * (K + 4) times the sum of the magnitudes, and
    the result by its last place."""
    T = len(latents)
    dtype = np.asarray(log_weights[-1]).dtype

    def last_place(v):      # of the rounding to the dtype: float64 results are not rounded again
        if dtype == np.float64:
            return np.zeros(v.shape)
        return np.where(np.isfinite(v), np.spacing(np.abs(np.where(np.isfinite(v), v, 0)).astype(dtype)), 0).astype(np.float64)

    def feature(function, time, latent):
        latent = np.asarray(latent)
        value = latent if function is None else np.asarray(function(time, latent))
        if value.shape[:2] != latent.shape[:2]:
            raise ValueError("a feature must be [batch_size, num_particles, ...], got {}".format(value.shape))
        return value.reshape(value.shape[0], value.shape[1], -1)

    smoothed, tolerance = [None] * T, [None] * T
    expectations, expectation_tolerance = [None] * (T - 1), [None] * (T - 1)
    log_w = np.asarray(log_weights[-1]).astype(np.float64)
    top = log_w.max(axis=1, keepdims=True)
    lse = top + np.log(np.exp(log_w - top).sum(axis=1, keepdims=True))
    smoothed[-1] = (log_w - lse).astype(dtype)
    tolerance[-1] = 4.0 * float(np.finfo(dtype).eps) * (np.abs(lse) + np.abs(log_w - lse))
    for t in range(T - 2, -1, -1):
        loc, nxt, log_w = locations(t), latents[t + 1], log_weights[t]
        f = feature(previous, t, latents[t]).astype(dtype)
        g = feature(following, t + 1, nxt).astype(np.float64)
        mean, den, _ = pairwise_mean(nxt, loc, scale, log_w, f)
        mean, den = mean.astype(dtype), den.astype(dtype)
        out = pairwise_lse(loc, nxt, scale, smoothed[t + 1], den, log_w)[0].astype(dtype)
        smoothed[t] = out
        den_tolerance = pairwise_lse_bound(nxt, loc, scale, log_w) + last_place(den)
        tolerance[t] = (tolerance[t + 1].max(axis=1, keepdims=True) + den_tolerance.max(axis=1, keepdims=True) +
                        pairwise_lse_bound(loc, nxt, scale, smoothed[t + 1], den, log_w) + last_place(out))
        weight = np.exp(smoothed[t + 1].astype(np.float64))
        m64 = mean.astype(np.float64)
        value = np.einsum("bj,bjq,bjp->bqp", weight, g, m64)
        expectations[t] = value.astype(dtype)
        mean_tolerance = pairwise_mean_bound(nxt, loc, scale, log_w, f) + last_place(mean)
        tau = tolerance[t + 1]
        moved = mean_tolerance + np.abs(m64) * (2.0 * tau * (1.0 + tau) + (nxt.shape[1] + 4) * EPSILON)[:, :, None]
        expectation_tolerance[t] = np.einsum("bj,bjq,bjp->bqp", weight, np.abs(g), moved) + last_place(value)
    if return_tolerance:
        return expectations, smoothed, (expectation_tolerance, tolerance)
    return expectations, smoothed


# ---- the MAP trajectory (particle Viterbi; Godsill, Doucet & West 2001): the max-plus twin of the marginal smoother ---------
NEAR_THE_ARGMAX = 1.0      # columns further below a row point's maximum cannot become it by rounding


def pairwise_argmax(rows, cols, scale, col_a, col_sub=None, row_add=None):
    """Operands as `pairwise_lse` takes them -> (out float64 [B,R], arg int64 [B,R], flags):

        s[b,r,c] = term[b,c] - 1/2 sum_d ((rows[b,r,d] - cols[b,c,d]) / scale[d])^2          (term as pairwise_lse forms it)
        out[b,r] = row_add[b,r] + max_c s[b,r,c]
        arg[b,r] = the SMALLEST c with s[b,r,c] == max_c s[b,r,c]

    in float64 whatever the operands' dtype is.  Conventions, per row point (row points and batch rows never affect one
    another); arg == C means "no column":
      a NaN among the row point's scores or in its row_add: FLAG_NAN_LOG_WEIGHT, out NaN, arg C;
      else a largest score of +inf: FLAG_DEGENERATE_ROW, out +inf, arg C;
      else every score -inf: out -inf, arg C and no flag — a point nothing reaches."""
    rows, cols, inv, col_a, col_sub, row_add = _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add)
    B, R = rows.shape[:2]
    C = cols.shape[1]
    out = np.empty((B, R), dtype=np.float64)
    arg = np.empty((B, R), dtype=np.int64)
    flags = 0
    for b in range(B):
        s, _, _ = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        add = np.zeros(R) if row_add is None else row_add[b]
        nan = np.isnan(s).any(axis=1) | np.isnan(add)
        held = np.where(np.isnan(s), -np.inf, s)
        smax, first = held.max(axis=1), held.argmax(axis=1)          # (argmax: the first of equal values)
        finite = np.isfinite(smax) & ~nan
        with np.errstate(invalid="ignore"):
            value = np.where(finite, add + np.where(finite, smax, 0.0), smax)      # +inf and -inf as they are
        out[b] = np.where(nan, np.nan, value)
        arg[b] = np.where(finite, first, C)
        if nan.any():
            flags |= FLAG_NAN_LOG_WEIGHT
        if (~nan & (smax == np.inf)).any():
            flags |= FLAG_DEGENERATE_ROW
    return out, arg, flags


def pairwise_argmax_bound(rows, cols, scale, col_a, col_sub=None, row_add=None):
    """[B,R] float64: how far a float64 evaluation of `pairwise_argmax`'s `out` in another order (fused against separately
    rounded multiply-adds, another order of the D additions, a reciprocal scale against a true division) may lie from
    this one, derived and not measured.  With eps = 2^-52 = 2 u (u the unit roundoff) and D values per point

        bound[b,r] = eps * ( (D + 4) * max_c (|term[b,c]| + q[r,c] / 2)  +  4 )  +  eps * |out[b,r]|

    the maximum over the columns whose score lies within 1 of the row point's largest.  The derivation, to first order,
    for one score s = term - q / 2 with q = sum_d t_d, t_d = ((r_d - c_d) / scale_d)^2:
      * term = col_a - col_sub is one float64 subtraction of the same two numbers in every evaluation: no difference;
      * the D products and D - 1 additions of q cost at most D u q in either of two evaluations, whether a product is
        rounded before it is added or fused into the addition, and in any order (every partial sum is at most q): the two
        differ by at most 2 D u q = D eps q, and the score by half of that, D eps q / 2;
      * the scaled difference is (r_d - c_d) * (1 / scale_d) in one evaluation (two roundings after the subtraction's) and
        (r_d - c_d) / scale_d in another (one): they differ by at most 3 u relatively, their squares by 6 u = 3 eps, the
        score by 3 eps q / 2;
      * the last step, term - q / 2, is one rounding in either evaluation (the halving is exact): eps |s| <= eps (|term| +
        q / 2) between the two.
    Together eps ((D + 3) q / 2 + |term| + q / 2) <= eps (D + 4) (|term| + q / 2).  The maximum of scores that each move by at
    most x moves by at most x, and only columns that can be the maximum of either evaluation count: those within
    NEAR_THE_ARGMAX = 1 of it, far more than any rounding.  The terms of second order are at most ((D + 4) eps)^2 times
    the same size: below the `+ 4` eps for every D <= 256 while the size stays under 4 / (260^2 eps) = 2.6e11.  The
    addition of row_add is one rounding in either evaluation, eps |out| between the two.  No sum over c: no C term.
    Zero where the result is not finite (those are conventions, held exactly)."""
    out, _, _ = pairwise_argmax(rows, cols, scale, col_a, col_sub, row_add)
    rows, cols, inv, col_a, col_sub, row_add = _pairwise_operands(rows, cols, scale, col_a, col_sub, row_add)
    B, R, D = rows.shape
    bound = np.zeros((B, R), dtype=np.float64)
    for b in range(B):
        s, term, q = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        with np.errstate(invalid="ignore"):
            smax = np.max(np.where(np.isnan(s), -np.inf, s), axis=1)
            finite = np.isfinite(smax) & np.isfinite(out[b])
            near = s >= (smax - NEAR_THE_ARGMAX)[:, None]
            size = np.where(near, np.abs(term)[None, :] + 0.5 * q, 0.0).max(axis=1)
        size = np.where(finite, size, 0.0)
        bound[b] = np.where(finite, EPSILON * ((D + 4) * size + 4 + np.abs(np.where(finite, out[b], 0.0))), 0.0)
    return bound


def pairwise_argmax_gap(rows, cols, scale, col_a, col_sub=None):
    """[B,R] float64: the winner's score minus the runner-up's (the largest score of any OTHER column; 0 for a tie, +inf
    with one column or where every other column is absent), NaN where `pairwise_argmax` gives no column.  What decides
    whether `arg` may be demanded exactly of an evaluation that is held to `pairwise_argmax_bound`: a gap above twice
    the bound leaves no choice."""
    _, arg, _ = pairwise_argmax(rows, cols, scale, col_a, col_sub)
    rows, cols, inv, col_a, col_sub, _ = _pairwise_operands(rows, cols, scale, col_a, col_sub, None)
    B, R = rows.shape[:2]
    C = cols.shape[1]
    gap = np.full((B, R), np.nan)
    for b in range(B):
        s, _, _ = _pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])
        for r in np.flatnonzero(arg[b] < C):
            others = np.delete(s[r], arg[b, r])
            with np.errstate(invalid="ignore"):
                gap[b, r] = s[r, arg[b, r]] - (others.max() if others.size else -np.inf)
    return gap


def viterbi_pass(latents, initial_log_prob, emission_log_probs, locations, scale, return_tolerance=False):
    """The whole MAP recursion (max-product over the stored particles), in float64 whatever the operands' dtype is:
    latents T x [B,K_t,...], initial_log_prob [B,K_0] = log mu(x[0]), emission_log_probs T x [B,K_t] = log g(y_t | x[t]),
    locations(t) -> the transition's location [B,K_t,...] of step t's stored particles for time t+1, scale one value or
    one per latent dimension.

        delta[0][i] = log mu(x[0][i]) + log g(y_0 | x[0][i])
        delta[t][j] = log g(y_t | x[t][j]) + cst + max_i ( delta[t-1][i] - 1/2 |x[t][j] - loc[t-1][i]|^2 )
        psi[t][j]   = the arg of that max                            (one pairwise_argmax; |.|^2 in units of the scale)
        cst         = - sum_d log scale[d] - D/2 log(2 pi)
        i[T-1] = argmax delta[T-1] (the smallest index),   i[t-1] = psi[t][i[t]]

    Returns (indices T x int64 [B], log_joint float64 [B]): the stored particle the most probable path passes through at
    every step, and log p(x*_{0..T-1}, y_{0..T-1}) of that path = max delta[T-1].  An index equal to the step's particle
    count means "no path" (log_joint is then not finite).
    `return_tolerance`: also (tolerance T x [B,K_t] float64, margin [B] float64).  The tolerance says how far an
    evaluation that keeps every launch within `pairwise_argmax_bound` may lie from this one's delta: max-plus moves by
    at most the largest move of its terms, so a step's tolerance is the largest of the step before plus its own bound
    plus what forming its row_add may differ by — four units in the last place of sum_d |log scale[d]| + D/2 log(2 pi)
    (another log) and of row_add itself; the first step is one addition of the same two numbers (one unit in the last
    place is granted).  log_joint's is the largest of the last step's.  The margin is the smallest gap between winner
    and runner-up over the choices that make the path — the final argmax and the psi look-ups ON the best path: while it
    exceeds twice the largest tolerance, every such evaluation finds the same path."""
    T = len(latents)
    wide = lambda v: np.asarray(v).astype(np.float64)
    x = [wide(latent) for latent in latents]
    B = x[0].shape[0]
    D = int(np.prod(x[0].shape[2:], dtype=np.int64))
    scale64 = np.broadcast_to(wide(scale).reshape(-1), (D,))
    log_scales, half_log_2pi = np.log(scale64), 0.5 * D * np.log(2.0 * np.pi)
    cst = -log_scales.sum() - half_log_2pi
    cst_slack = 4.0 * EPSILON * (np.abs(log_scales).sum() + half_log_2pi)

    delta, psi, tolerance = [None] * T, [None] * T, [None] * T
    delta[0] = wide(initial_log_prob) + wide(emission_log_probs[0])
    with np.errstate(invalid="ignore"):
        tolerance[0] = EPSILON * np.where(np.isfinite(delta[0]), np.abs(delta[0]), 0.0)
    for t in range(1, T):
        loc = wide(locations(t - 1))
        row_add = wide(emission_log_probs[t]) + cst
        delta[t], psi[t], _ = pairwise_argmax(x[t], loc, scale64, delta[t - 1], None, row_add)
        own = pairwise_argmax_bound(x[t], loc, scale64, delta[t - 1], None, row_add)
        with np.errstate(invalid="ignore"):
            forming = cst_slack + 4.0 * EPSILON * np.where(np.isfinite(row_add), np.abs(row_add), 0.0)
        tolerance[t] = tolerance[t - 1].max(axis=1, keepdims=True) + own + forming
    nothing = np.zeros((B, 1, 0))
    last = delta[-1]
    log_joint, final, _ = pairwise_argmax(nothing, np.zeros((B, last.shape[1], 0)), None, last)
    log_joint, final = log_joint[:, 0], final[:, 0]
    margin = pairwise_argmax_gap(nothing, np.zeros((B, last.shape[1], 0)), None, last)[:, 0]
    indices = [None] * T
    indices[-1] = final
    rows_of = np.arange(B)
    for t in range(T - 1, 0, -1):
        at = np.minimum(indices[t], x[t].shape[1] - 1)          # ("no column" is clamped, never dereferenced)
        previous = psi[t][rows_of, at]
        indices[t - 1] = np.where(indices[t] < x[t].shape[1], previous, x[t - 1].shape[1])
        chosen = x[t][rows_of, at][:, None]                     # [B,1,...]: the path's particle of step t
        gap = pairwise_argmax_gap(chosen, wide(locations(t - 1)), scale64, delta[t - 1])[:, 0]
        margin = np.minimum(margin, gap)                        # (NaN where there is no path: it stays NaN)
    if return_tolerance:
        return indices, log_joint, (tolerance, margin)
    return indices, log_joint
