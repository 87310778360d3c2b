"""NumPy statement (float64) of the CONTRACT of the fully adapted auxiliary particle filter (Pitt & Shephard 1999): the gain
algebra `aesmc_amd.adapted.gains` forms on the host, the two kernels around the resampling launch
(include/aesmc_hip.h: aesmc_affine_quadratic_logweight, K27, and aesmc_adapted_draw, K28) with the bounds they are held
to, the whole filter that `aesmc_amd.adapted.adapted_filter` makes of them, and the Kalman filter it is measured against.
Written without regard to the kernels' structure (no tiles, no tables).

Transition N(mu(x_{t-1}), S_f), S_f = diag(s_f^2); emission N(C x_t + d, S_g), S_g = diag(s_g^2).  Then

    p(y_t | x_{t-1})       = N(y_t; C mu + d, S),   S = C S_f C^T + S_g
    p(x_t | x_{t-1}, y_t)  = N(mu + G (y_t - d - C mu), S_f - G C S_f),   G = S_f C^T S^-1

and with chol(S) = Lam Lam^T, W = Lam^-1, P = -W C, M = I - G C, chol(S_f - G C S_f) = L L^T, o = W (y - d), r = G (y - d):

    log p(y_t | x_{t-1}) = base - 1/2 |P mu + o|^2,   base = -Dy/2 log 2 pi - sum_j log Lam_jj
    x_t = r + M mu + L eps,   eps ~ N(0, I).

(This package never imports the oracle — tests/test_library.py.)
"""
import numpy as np

FLAG_NAN_LOG_WEIGHT = 1
FLAG_DEGENERATE_ROW = 2
FLAG_INDEX_OUT_OF_RANGE = 4

UNIT = 2.0 ** -53      # the unit roundoff of float64
_LOG_2PI = 1.8378770664093453


def _diagonal(scale, size):
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if scale.size not in (1, size):
        raise ValueError("a scale of {} values for {} dimensions".format(scale.size, size))
    return np.broadcast_to(scale, (size,)) ** 2


def gains(transition_scale, weight, emission_scale):
    """The float64 operands of one (s_f, C, s_g): a dict with P [Dy,D], M [D,D], L [D,D] (lower triangular), W [Dy,Dy],
    G [D,Dy] and base.  transition_scale: one value or D; weight: C [Dy,D]; emission_scale: one value or Dy.
    np.linalg.LinAlgError when a covariance has no Cholesky factor."""
    C = np.asarray(weight, dtype=np.float64)
    Dy, D = C.shape
    var_f, var_g = _diagonal(transition_scale, D), _diagonal(emission_scale, Dy)
    S = (C * var_f) @ C.T + np.diag(var_g)
    lam = np.linalg.cholesky(S)
    W = np.linalg.solve(lam, np.eye(Dy))
    G = (var_f[:, None] * C.T) @ (W.T @ W)
    sigma = np.diag(var_f) - G @ (C * var_f)
    L = np.linalg.cholesky(0.5 * (sigma + sigma.T))
    return {"P": -W @ C, "M": np.eye(D) - G @ C, "L": L, "W": W, "G": G,
            "base": float(-0.5 * Dy * _LOG_2PI - np.log(np.diag(lam)).sum())}


def row_offsets(gain, observation, emission_offset=None):
    """(o [B,Dy], r [B,D]) of `gains`' dict for observations [B,Dy] and an emission offset None, [Dy] or [B,Dy]."""
    residual = np.asarray(observation, dtype=np.float64)
    if emission_offset is not None:
        residual = residual - np.asarray(emission_offset, dtype=np.float64)
    return residual @ gain["W"].T, residual @ gain["G"].T


# ---- K27 -------------------------------------------------------------------------------------------------------------------
def affine_quadratic_logweight(loc, P, offset, base):
    """out[b,k] = base - 1/2 sum_j r_j^2, r_j = offset[b,j] + sum_i P[j,i] loc[b,k,i]: i ascending from the offset, j
    ascending from zero, in float64, rounded once to loc's dtype.  loc [B,K,D] (any broadcast view), P [Dy,D], offset
    [B,Dy].  A NaN location gives a NaN log-weight."""
    loc = np.asarray(loc)
    x = loc.astype(np.float64)
    P, offset = np.asarray(P, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    B, K, D = x.shape
    q = np.zeros((B, K))
    for j in range(P.shape[0]):
        r = np.broadcast_to(offset[:, None, j], (B, K)).copy()
        for i in range(D):
            r = r + P[j, i] * x[:, :, i]
        q = q + r * r
    return (base - 0.5 * q).astype(loc.dtype)


def affine_quadratic_logweight_bound(loc, P, offset, base):
    """[B,K] float64: how far a float64 evaluation of `affine_quadratic_logweight` with fused multiply-adds (the kernel's)
    may lie from this one with separately rounded ones, derived and not measured.  With u = 2^-53, A_j = |offset_j| +
    sum_i |P_ji loc_i| (which bounds |r_j|) and each evaluation's own error against the exact value:

        dr_j  = (D + 1) u A_j                                        D additions, the products rounded (or not)
        dq    = sum_j (2 A_j dr_j + dr_j^2) + (Dy + 1) u sum_j (A_j + dr_j)^2
        bound = 2 * 1.01 * ( dq / 2 + 2 u (|base| + sum_j (A_j + dr_j)^2 / 2) )

    (twice: two evaluations; 1.01: the terms of second order)."""
    x = np.abs(np.asarray(loc).astype(np.float64))
    P, offset = np.abs(np.asarray(P, dtype=np.float64)), np.abs(np.asarray(offset, dtype=np.float64))
    Dy, D = P.shape
    A = offset[:, None, :] + x @ P.T                                  # [B,K,Dy]
    dr = (D + 1) * UNIT * A
    size = ((A + dr) ** 2).sum(axis=2)
    dq = (2 * A * dr + dr * dr).sum(axis=2) + (Dy + 1) * UNIT * size
    return 2 * 1.01 * (0.5 * dq + 2 * UNIT * (abs(base) + 0.5 * size))


# ---- K28 -------------------------------------------------------------------------------------------------------------------
def adapted_draw(loc, idx, M, offset, L, eps):
    """(out [B,K,D] in eps' dtype, flags): with a = idx[b,k] (None: k), out[b,k,j] = offset[b,j] + sum_{i<D} M[j,i]
    loc[b,a,i] + sum_{i<=j} L[j,i] eps[b,k,i], added in that order in float64 and rounded once.  An `a` outside [0, K)
    gives NaN for that particle's D values and FLAG_INDEX_OUT_OF_RANGE."""
    eps = np.asarray(eps)
    B, K, D = eps.shape
    x = np.broadcast_to(np.asarray(loc), (B, K, D)).astype(np.float64)
    M, L = np.asarray(M, dtype=np.float64), np.asarray(L, dtype=np.float64)
    offset = np.asarray(offset, dtype=np.float64)
    flags = 0
    bad = np.zeros((B, K), dtype=bool)
    if idx is not None:
        idx = np.asarray(idx)
        bad = (idx < 0) | (idx >= K)
        if bad.any():
            flags |= FLAG_INDEX_OUT_OF_RANGE
        x = np.take_along_axis(x, np.where(bad, 0, idx)[:, :, None], axis=1)
    e = eps.astype(np.float64)
    acc = np.broadcast_to(offset[:, None, :], (B, K, D)).copy()
    for i in range(D):
        acc += M[None, None, :, i] * x[:, :, i:i + 1]
    for i in range(D):
        acc[:, :, i:] += L[None, None, i:, i] * e[:, :, i:i + 1]
    acc[bad] = np.nan
    return acc.astype(eps.dtype), flags


def adapted_draw_bound(loc, idx, M, offset, L, eps):
    """[B,K,D] float64: the counterpart of `affine_quadratic_logweight_bound` for `adapted_draw`.  Element j is a chain of
    D + j + 1 additions over terms of total magnitude A_j = |offset_j| + sum_i |M_ji loc_i| + sum_{i<=j} |L_ji eps_i|:

        bound_j = 2 * 1.01 * (D + j + 2) u A_j        (zero where the index is out of range)."""
    eps = np.asarray(eps)
    B, K, D = eps.shape
    sized, _ = adapted_draw(np.abs(np.asarray(loc)).astype(np.float64), idx, np.abs(np.asarray(M, dtype=np.float64)),
                            np.abs(np.asarray(offset, dtype=np.float64)), np.abs(np.asarray(L, dtype=np.float64)),
                            np.abs(eps).astype(np.float64))
    bound = 2 * 1.01 * (D + np.arange(D) + 2)[None, None, :] * UNIT * sized
    return np.where(np.isnan(bound), 0.0, bound)


# ---- the resampling step (K2's contract, both schemes) and the whole filter -------------------------------------------------
def ancestor_index(log_w, u):
    """(idx int64 [B,K], row log-sum-exp float64 [B], flags, margin): K2's contract — w = exp(log_w - max), c = the
    running sum of w over its total, idx[b,k] = #{j : c[j] <= pos[k]} with pos[k] = (u[b] + k) / K (u [B]: systematic) or
    (u[b,k] + k) / K (u [B,K]: stratified).  A NaN row: FLAG_NAN_LOG_WEIGHT, a row without a finite maximum:
    FLAG_DEGENERATE_ROW, idx = K.  `margin`: the smallest |c[j] - pos[k]| over the good rows (inf: none) — the device sums
    the same weights in another association, and only an index whose position lies this close to a step of the running
    sum can differ."""
    log_w = np.asarray(log_w).astype(np.float64)
    B, K = log_w.shape
    u = np.asarray(u, dtype=np.float64)
    u = np.broadcast_to(u.reshape(B, 1), (B, K)) if u.size == B and u.shape != (B, K) else u.reshape(B, K)
    idx = np.full((B, K), K, dtype=np.int64)
    lse = np.full(B, np.nan)
    flags, margin = 0, np.inf
    for b in range(B):
        row = log_w[b]
        if np.isnan(row).any():
            flags |= FLAG_NAN_LOG_WEIGHT
            continue
        top = row.max()
        if not np.isfinite(top):
            flags |= FLAG_DEGENERATE_ROW
            lse[b] = top
            continue
        w = np.exp(row - top)
        c = np.cumsum(w)
        lse[b] = top + np.log(c[-1])
        c = c / c[-1]
        pos = (u[b] + np.arange(K)) / K
        idx[b] = np.searchsorted(c, pos, side="right")
        margin = min(margin, np.abs(c[None, :] - pos[:, None]).min())
    return idx, lse, flags, margin


def adapted_pass(observations, loc0, scale0, location, transition_scale, weight, emission_offset, emission_scale,
                 noise, uniforms, dtype=np.float64, lipschitz=1.0):
    """The whole filter.  observations: T x [B,Dy]; loc0 [D] or [B,D], scale0 one value or D; location(x [B,K,D], t) ->
    the transition's location [B,K,D] for time t of the stored particles x of time t-1; transition_scale, weight (C
    [Dy,D]), emission_offset (None, [Dy] or [B,Dy]), emission_scale: the model; noise: T x [B,K,D] standard-normal draws;
    uniforms: T-1 x [B] (systematic) or [B,K] (stratified); dtype: what the particles and first-stage weights are rounded
    to, as the device's launches round theirs.

    Returns a dict: log_marginal_likelihood [B] float64, latents (T x [B,K,D]), ancestral_indices ((T-1) x int64 [B,K]),
    first_stage_log_weights ((T-1) x [B,K]), flags, margins (T-1 floats: `ancestor_index`'s, the guard under which the
    device's indices must equal these), and tolerances: `latents` (T floats) and `log_marginal_likelihood` (one float),
    how far a device run whose launches stay within their bounds may lie from this one, given that the location is
    `lipschitz`-Lipschitz in the sup norm and evaluated to 4 (D + 2) u (lipschitz max|x| + 1):

        tol_mu[t]   = lipschitz tol_x[t-1] + 4 (D + 2) u (lipschitz max|x[t-1]| + 1)
        tol_x[t]    = |M|_inf tol_mu[t] + max adapted_draw_bound + (float32: one unit in the last place of the largest |x|)
        tol_lam[t]  = max_k sum_j A_j |P|_j,1 tol_mu[t] + max bound + (float32: one unit in the last place)
        tol_Z      += tol_lam[t] + (K + 4) u (1 + |lse| + log K)                 (a log-sum-exp moves by at most its terms;
                                                                                  float32: two units in its last place)
    """
    T = len(observations)
    noise = [np.asarray(e) for e in noise]
    B, K, D = noise[0].shape
    single = np.dtype(dtype) == np.float32
    last_place = (lambda v: float(np.spacing(np.float32(np.abs(v).max())))) if single else (lambda v: 0.0)
    step = gains(transition_scale, weight, emission_scale)
    first = gains(scale0, weight, emission_scale)
    loc0 = np.broadcast_to(np.asarray(loc0, dtype=np.float64), (B, D))
    o, r = row_offsets(first, observations[0], emission_offset)
    residual = loc0 @ first["P"].T + o
    log_z = first["base"] - 0.5 * (residual * residual).sum(axis=1)
    start = loc0[:, None, :].astype(dtype)
    x, flags = adapted_draw(start, None, first["M"], r, first["L"], noise[0].astype(dtype))
    tol_x = [float(adapted_draw_bound(start, None, first["M"], r, first["L"], noise[0].astype(dtype)).max()) + last_place(x)]
    tol_z = 8 * (first["P"].shape[0] + D + 4) * UNIT * (abs(first["base"]) + (np.abs(loc0) @ np.abs(first["P"]).T +
                                                                                np.abs(o)).max() ** 2 * first["P"].shape[0])
    latents, ancestors, stages, margins = [x], [], [], []
    norm_m = np.abs(step["M"]).sum(axis=1).max()
    row_p = np.abs(step["P"]).sum(axis=1)
    for t in range(1, T):
        mu = np.asarray(location(latents[-1], t)).astype(dtype)
        tol_mu = lipschitz * tol_x[-1] + 4 * (D + 2) * UNIT * (lipschitz * np.abs(latents[-1]).max() + 1.0)
        o, r = row_offsets(step, observations[t], emission_offset)
        lam = affine_quadratic_logweight(mu, step["P"], o, step["base"])
        A = np.abs(o)[:, None, :] + np.abs(mu.astype(np.float64)) @ np.abs(step["P"]).T
        tol_lam = float((A * row_p).sum(axis=2).max()) * tol_mu * 1.01 + \
            float(affine_quadratic_logweight_bound(mu, step["P"], o, step["base"]).max()) + last_place(lam)
        idx, lse, bits, margin = ancestor_index(lam, uniforms[t - 1])
        flags |= bits
        log_z = log_z + lse - np.log(K)
        tol_z += tol_lam + (K + 4) * UNIT * (1.0 + float(np.abs(lse).max()) + np.log(K)) + 2 * last_place(lse)
        eps = noise[t].astype(dtype)
        x, bits = adapted_draw(mu, idx, step["M"], r, step["L"], eps)
        flags |= bits
        tol_x.append(norm_m * tol_mu * 1.01 + float(adapted_draw_bound(mu, idx, step["M"], r, step["L"], eps).max()) +
                     last_place(x))
        latents.append(x), ancestors.append(idx), stages.append(lam), margins.append(margin)
    return {"log_marginal_likelihood": log_z, "latents": latents, "ancestral_indices": ancestors,
            "first_stage_log_weights": stages, "flags": flags, "margins": margins,
            "tolerances": {"latents": tol_x, "log_marginal_likelihood": float(tol_z)}}


def bootstrap_pass(observations, loc0, scale0, transition_weight, transition_scale, weight, emission_scale, num_particles,
                   rng):
    """log Z-hat [B] of a NumPy bootstrap filter (proposal = transition, the initial at time 0; systematic resampling at
    every step) for the linear model x_t ~ N(A x_{t-1}, s_f^2), y_t ~ N(C x_t, s_g^2): what the adapted filter's variance
    is measured against."""
    A, C = np.asarray(transition_weight, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    Dy, D = C.shape
    B, K = np.asarray(observations[0]).shape[0], num_particles
    s_f, s_g = np.sqrt(_diagonal(transition_scale, D)), np.sqrt(_diagonal(emission_scale, Dy))
    s_0 = np.sqrt(_diagonal(scale0, D))
    log_z = np.zeros(B)
    x = np.asarray(loc0, dtype=np.float64) + s_0 * rng.standard_normal((B, K, D))
    for t, y in enumerate(observations):
        if t > 0:
            idx = ancestor_index(log_w, rng.uniform(size=B))[0]
            x = np.take_along_axis(x, idx[:, :, None], axis=1) @ A.T + s_f * rng.standard_normal((B, K, D))
        z = (np.asarray(y, dtype=np.float64)[:, None, :] - x @ C.T) / s_g
        log_w = -0.5 * (z * z).sum(axis=2) - np.log(s_g).sum() - 0.5 * Dy * _LOG_2PI
        top = log_w.max(axis=1)
        log_z += top + np.log(np.exp(log_w - top[:, None]).mean(axis=1))
    return log_z


def kalman_filter(A, C, s_f, s_g, loc0, scale0, ys):
    """The exact filter of x_0 ~ N(loc0, diag(scale0^2)), x_t ~ N(A x_{t-1}, diag(s_f^2)), y_t ~ N(C x_t, diag(s_g^2)) for
    ys: T x [B,Dy] (or T x [Dy]: one sequence).  Returns (filtered means [T,B,D], filtered covariances [T,D,D],
    log p(y_0..y_{T-1}) [B]); without the batch dimension when ys has none."""
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    Dy, D = C.shape
    ys = [np.asarray(y, dtype=np.float64) for y in ys]
    batched = ys[0].ndim == 2
    if not batched:
        ys = [y[None, :] for y in ys]
    B = ys[0].shape[0]
    Q, R = np.diag(_diagonal(s_f, D)), np.diag(_diagonal(s_g, Dy))
    mean = np.broadcast_to(np.asarray(loc0, dtype=np.float64), (B, D)).copy()
    cov = np.diag(_diagonal(scale0, D))
    means, covs, total = [], [], np.zeros(B)
    for t, y in enumerate(ys):
        if t > 0:
            mean, cov = mean @ A.T, A @ cov @ A.T + Q
        S = C @ cov @ C.T + R
        residual = y - mean @ C.T
        solved = np.linalg.solve(S, residual.T).T
        total += -0.5 * ((residual * solved).sum(axis=1) + np.linalg.slogdet(S)[1] + Dy * _LOG_2PI)
        gain = cov @ C.T @ np.linalg.inv(S)
        mean, cov = mean + residual @ gain.T, cov - gain @ C @ cov
        means.append(mean.copy()), covs.append(cov.copy())
    means, covs = np.stack(means), np.stack(covs)
    return (means, covs, total) if batched else (means[:, 0], covs, total[0])


# ---- K29 / K30: the adjoints of the two launches ------------------------------------------------------------------------
def _unit_of(dtype):
    """The unit roundoff of the particles' dtype (what one rounding to T costs, relative)."""
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else UNIT


def affine_quadratic_logweight_backward(loc, P, offset, grad):
    """(grad_loc [B,K,D] in loc's dtype, grad_P float64 [Dy,D], grad_offset float64 [B,Dy]) of `affine_quadratic_logweight`
    for the gradient grad [B,K] arriving at its output, from plain float64 matrix products: with rho = loc P^T + offset
    and w = -grad rho,  grad_loc = w P,  grad_P = sum_{b,k} w (outer) loc,  grad_offset = sum_k w.  (The gradient of
    `base` is grad.sum().)"""
    loc = np.asarray(loc)
    x = loc.astype(np.float64)
    P, offset = np.asarray(P, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    g = np.asarray(grad).astype(np.float64)
    w = -g[:, :, None] * (x @ P.T + offset[:, None, :])
    return (w @ P).astype(loc.dtype), np.einsum("bkj,bki->ji", w, x), w.sum(axis=1)


def affine_quadratic_logweight_backward_bound(loc, P, offset, grad):
    """(bound of grad_loc [B,K,D], of grad_P [Dy,D], of grad_offset [B,Dy]), float64: how far the kernel's outputs may
    lie from `affine_quadratic_logweight_backward`'s, derived and not measured.  u = 2^-53, u_T the unit roundoff of loc's
    dtype, A_j = |offset_j| + sum_i |P_ji loc_i| (which bounds |rho_j|), |w_j| <= |grad| A_j, and w_j itself is a chain of
    D additions and one product: off by at most (D + 2) u |grad| A_j from the exact value.

        grad_loc_i     a chain of Dy multiply-adds over terms of total size T_i = sum_j |grad| A_j |P_ji|:
                       2 * 1.01 * (Dy + 1 + D + 2) u T_i  +  2 u_T T_i          (two evaluations; each rounds once to T)
        grad_P_ji      a sum of B K terms in any order, each a chain of D + 2 operations:
                       2 * 1.01 * (B K + D + 2) u sum_{b,k} |grad| A_j |loc_i|
        grad_offset_bj 2 * 1.01 * (K + D + 2) u sum_k |grad| A_j"""
    loc = np.asarray(loc)
    x = np.abs(loc.astype(np.float64))
    P, offset = np.abs(np.asarray(P, dtype=np.float64)), np.abs(np.asarray(offset, dtype=np.float64))
    g = np.abs(np.asarray(grad).astype(np.float64))
    B, K, D = x.shape
    Dy = P.shape[0]
    size = g[:, :, None] * (offset[:, None, :] + x @ P.T)                     # |grad| A_j  [B,K,Dy]
    chain = size @ P
    bound_loc = 2 * 1.01 * (Dy + D + 3) * UNIT * chain + 2 * _unit_of(loc.dtype) * chain
    bound_P = 2 * 1.01 * (B * K + D + 2) * UNIT * np.einsum("bkj,bki->ji", size, x)
    bound_offset = 2 * 1.01 * (K + D + 2) * UNIT * size.sum(axis=1)
    return bound_loc, bound_P, bound_offset


def adapted_draw_backward(loc, idx, M, L, eps, grad):
    """(h [B,K,D] in eps' dtype, grad_M [D,D], grad_L [D,D], grad_r [B,D] float64, flags) of `adapted_draw` for the
    gradient grad [B,K,D] arriving at its output, from plain float64 matrix products: with a = idx[b,k] (None: k),
    h = grad M (the gradient of the gathered row loc[b,a]),  grad_M = sum_{b,k} grad (outer) loc[b,a],  grad_L = the lower
    triangle of sum_{b,k} grad (outer) eps (exactly zero above the diagonal),  grad_r = sum_k grad.  L is taken for its
    shape only.  An `a` outside [0, K) contributes nothing to the three sums, gives a NaN row of h and
    FLAG_INDEX_OUT_OF_RANGE."""
    eps = np.asarray(eps)
    B, K, D = eps.shape
    x = np.broadcast_to(np.asarray(loc), (B, K, D)).astype(np.float64)
    M = np.asarray(M, dtype=np.float64)
    assert np.asarray(L).shape == (D, D)
    G = np.asarray(grad).astype(np.float64)
    flags = 0
    bad = np.zeros((B, K), dtype=bool)
    if idx is not None:
        idx = np.asarray(idx)
        bad = (idx < 0) | (idx >= K)
        if bad.any():
            flags |= FLAG_INDEX_OUT_OF_RANGE
        x = np.take_along_axis(x, np.where(bad, 0, idx)[:, :, None], axis=1)
    counted = np.where(bad[:, :, None], 0.0, G)
    x = np.where(bad[:, :, None], 0.0, x)
    h = G @ M
    h[bad] = np.nan
    grad_M = np.einsum("bkj,bki->ji", counted, x)
    grad_L = np.tril(np.einsum("bkj,bki->ji", counted, eps.astype(np.float64)))
    return h.astype(eps.dtype), grad_M, grad_L, counted.sum(axis=1), flags


def adapted_draw_backward_bound(loc, idx, M, L, eps, grad):
    """(bound of h [B,K,D], of grad_M [D,D], of grad_L [D,D], of grad_r [B,D]), float64: the counterpart of
    `affine_quadratic_logweight_backward_bound`.  The operands enter exactly, so every term is one product:

        h_i        a chain of D multiply-adds over terms of total size T_i = sum_j |grad_j M_ji|:
                   2 * 1.01 * (D + 1) u T_i + 2 u_T T_i           (zero where the index is out of range: NaN there)
        grad_M_ji  2 * 1.01 * (B K + 1) u sum_{b,k} |grad_j loc[b,a]_i|      grad_L_ji likewise with eps, zero above the
        grad_r_bj  2 * 1.01 * (K + 1) u sum_k |grad_j|                       diagonal."""
    eps = np.asarray(eps)
    B, K, D = eps.shape
    sized = adapted_draw_backward(np.abs(np.asarray(loc)).astype(np.float64), idx, np.abs(np.asarray(M, dtype=np.float64)), L,
                                  np.abs(eps).astype(np.float64), np.abs(np.asarray(grad)).astype(np.float64))
    chain = np.where(np.isnan(sized[0]), 0.0, sized[0])
    bound_h = 2 * 1.01 * (D + 1) * UNIT * chain + 2 * _unit_of(eps.dtype) * chain
    factor = 2 * 1.01 * (B * K + 1) * UNIT
    return bound_h, factor * sized[1], factor * sized[2], 2 * 1.01 * (K + 1) * UNIT * sized[3]


# ---- the whole differentiable filter, restated in PyTorch ------------------------------------------------------------------
def adapted_elbo_restated(observations, loc0, scale0, location, transition_scale, weight, emission_offset, emission_scale,
                          noise, ancestors, dtype=None):
    """What `aesmc_amd.adapted.adapted_elbo` computes and differentiates, restated with torch.distributions, torch.linalg
    and torch.gather — no kernel, no `_ops` function, no provider — for GIVEN noise (T x [B,K,D]) and GIVEN ancestors
    ((T-1) x int64 [B,K], held fixed: they carry no gradient).  observations: T x [B,Dy]; loc0 [D] or [B,D]; scale0,
    transition_scale, emission_scale: tensors of one value or one per dimension; location(x [B,K,D], t) -> the transition's
    location of the stored particles x of time t-1 (a differentiable torch function); weight: C [Dy,D]; emission_offset:
    None, [Dy] or [B,Dy].  `dtype` (default torch.float64): what everything is computed in.  Any of the tensors may
    require grad.  Returns a dict: log_marginal_likelihood [B] (on the tape), latents (T x [B,K,D]).

        log p(y_t | x_{t-1}) = MultivariateNormal(C mu + d, C S_f C^T + S_g).log_prob(y_t)
        x_t = mu[a] + (y_t - d - C mu[a]) G^T + eps chol(S_f - G C S_f)^T,   G = S_f C^T S^-1   (torch.linalg.solve)"""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    cast = lambda t: None if t is None else t.to(dtype)
    C, d = cast(weight), cast(emission_offset)
    Dy, D = C.shape
    B, K = noise[0].shape[:2]
    variances = lambda scale, size: (cast(scale).reshape(-1) ** 2).expand(size)
    var_g = variances(emission_scale, Dy)

    def step(mu, var_f, y, eps, index):
        """(log p(y | x_{t-1}) [B,K], x_t [B,K,D]) for the locations mu [B,K,D] of the stored particles."""
        S = (C * var_f) @ C.t() + torch.diag(var_g)
        predicted = mu @ C.t() + (0.0 if d is None else (d.unsqueeze(1) if d.dim() == 2 else d))
        log_lambda = torch.distributions.MultivariateNormal(predicted, covariance_matrix=S, validate_args=False).log_prob(
            y.unsqueeze(1))
        G = torch.linalg.solve(S, C * var_f).t()                           # S_f C^T S^-1  [D,Dy]
        sigma = torch.diag(var_f) - G @ (C * var_f)
        chol = torch.linalg.cholesky(0.5 * (sigma + sigma.t()))
        if index is not None:
            expanded = index.unsqueeze(-1).expand(-1, -1, D)
            mu, predicted = torch.gather(mu, 1, expanded), torch.gather(predicted, 1, index.unsqueeze(-1).expand(-1, -1, Dy))
        x = mu + (y.unsqueeze(1) - predicted) @ G.t() + cast(eps) @ chol.t()
        return log_lambda, x

    ys = [cast(y) for y in observations]
    start = cast(loc0).expand(B, D).unsqueeze(1).expand(B, K, D)
    log_lambda, x = step(start, variances(scale0, D), ys[0], noise[0], None)
    log_z = log_lambda[:, 0]                                               # log p(y_0), exact
    latents = [x]
    var_f = variances(transition_scale, D)
    for t in range(1, len(ys)):
        log_lambda, x = step(location(latents[-1], t), var_f, ys[t], noise[t], ancestors[t - 1])
        log_z = log_z + torch.logsumexp(log_lambda, dim=1) - np.log(K)
        latents.append(x)
    return {"log_marginal_likelihood": log_z, "latents": latents}
