"""NumPy statement of the CONTRACT of the Rao-Blackwellised particle filter (mixture Kalman filter; Doucet, de Freitas,
Murphy & Russell 2000; Chen & Liu 2000) for switching linear-Gaussian state-space models: the one launch of a step
(include/aesmc_hip.h: aesmc_switching_kalman_step, K31) with the bound it is held to, the whole filter that
`aesmc_amd.rao_blackwell.switching_filter` makes of it and the resampling launch, and the exact likelihood by enumeration
it is measured against.  Written without regard to the kernel's structure (no tiles, no padding, no LDS).

    s_0 ~ Cat(pi0)                      s_t | s_{t-1} ~ Cat(Pi[s_{t-1}, :])
    z_0 ~ N(m0, diag(s0^2))             z_t = A[s_t] z_{t-1} + b[s_t] + N(0, diag(q[s_t]^2))
    y_t = C[s_t] z_t + d[s_t] + N(0, diag(r[s_t]^2))        (also at t = 0, under s_0)

Particle k of batch row b carries (s, m, P).  One step, per particle, every sum in ascending index order starting from the
value named first, every product rounded before it is added (the kernel fuses them: `switching_kalman_step_bound`):

    j        = idx[b,k] (None, or step 0: k)
    s        = #{ i < M-1 : cdf[regime[b,j], i] <= uniforms[b,k] }                    (step 0: the row cdf0)
    m-_i     = b_s[i] + sum_l A_s[i,l] m[b,j,l]                                       (step 0: m0)
    W_il     = 0 + sum_c A_s[i,c] P[b,j][c,l];    P-_ij = (i == j ? q_s[i]^2 : 0) + sum_l A_s[i,l] W_jl,   i >= j
                                                                                      (step 0: diag(s0^2))
    e_i      = (y[b,i] - d_s[i]) - sum_l C_s[i,l] m-_l
    U_il     = 0 + sum_c C_s[i,c] P-[c,l];        S_ij = (i == j ? r_s[i]^2 : 0) + sum_l C_s[i,l] U_jl,    i >= j
    Lam      = chol(S), column by column: Lam_jj = sqrt(S_jj - sum_{c<j} Lam_jc^2), rho_j = 1 / Lam_jj,
               Lam_ij = (S_ij - sum_{c<j} Lam_ic Lam_jc) rho_j
    v_i      = (e_i - sum_{c<i} Lam_ic v_c) rho_i;    V_il = (U_il - sum_{c<i} Lam_ic V_cl) rho_i
    log w    = (-1/2 sum_i v_i^2 - sum_j log Lam_jj) - Dy * (1/2 log 2 pi)
    m_l      = m-_l + sum_i V_il v_i;             P_lj = P-_lj - sum_i V_il V_ij,  l >= j    (the lower triangle, packed:
                                                                                      element (i,j) at i(i+1)/2 + j)

(This package never imports the oracle — tests/test_library.py.)
"""
import itertools

import numpy as np

from . import adapted as _adapted

FLAG_NAN_LOG_WEIGHT = 1
FLAG_DEGENERATE_ROW = 2
FLAG_INDEX_OUT_OF_RANGE = 4

UNIT = 2.0 ** -53      # the unit roundoff of float64
HALF_LOG_2PI = 0.9189385332046727
MAX_LATENT_DIM, MAX_OBSERVATION_DIM, MAX_REGIMES = 8, 8, 16


def tri(i, j):
    """Where element (i,j) of a symmetric matrix lies in its packed lower triangle."""
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


def pack(full):
    """[..., D, D] symmetric -> [..., D(D+1)/2]."""
    D = full.shape[-1]
    return np.stack([full[..., i, j] for i in range(D) for j in range(i + 1)], axis=-1)


def unpack(packed, D):
    """[..., D(D+1)/2] -> [..., D, D] symmetric."""
    full = np.empty(packed.shape[:-1] + (D, D), dtype=packed.dtype)
    for i in range(D):
        for j in range(D):
            full[..., i, j] = packed[..., tri(i, j)]
    return full


def cumulative(probabilities):
    """The cumulative rows the regime draw reads: float64 running sums along the last axis, the last entry set to 1."""
    rows = np.cumsum(np.asarray(probabilities, dtype=np.float64), axis=-1)
    rows[..., -1] = 1.0
    return rows


def operands(pi0, Pi, m0, s0, A, b, q, C, d, r):
    """The model as the step takes it: a dict of float64 arrays pi0 [M], Pi [M,M], cdf0 [M], cdf [M,M], m0 [D], s0 [D],
    A [M,D,D], b [M,D], q [M,D], C [M,Dy,D], d [M,Dy], r [M,Dy]; a leading extent of 1 in place of M (and one value in
    place of s0's D) is expanded."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    pi0, Pi, A, C = f(pi0), f(Pi), f(A), f(C)
    M, D, Dy = pi0.shape[0], A.shape[-1], C.shape[-2]
    grow = lambda x, shape: np.ascontiguousarray(np.broadcast_to(f(x), shape))
    return {"pi0": pi0, "Pi": Pi, "cdf0": cumulative(pi0), "cdf": cumulative(Pi), "m0": grow(m0, (D,)),
            "s0": grow(np.reshape(f(s0), -1), (D,)), "A": grow(A, (M, D, D)), "b": grow(b, (M, D)), "q": grow(q, (M, D)),
            "C": grow(C, (M, Dy, D)), "d": grow(d, (M, Dy)), "r": grow(r, (M, Dy))}


# ---- values that carry a bound on their own error -----------------------------------------------------------------------------
# A pair (v, e): the value as computed and a bound on |v - exact|, where "exact" is the same expression in real
# arithmetic on the same inputs.  e is None where no bound is wanted (the plain contract).
def _chain(start, terms, negate=False):
    """start + sum_i a_i b_i (negate: start - sum), one product and one addition at a time in order.  A chain of n terms
    evaluated in ANY mix of fused and separately rounded multiply-adds lies within (n + 1) u (|start| + sum |a_i b_i|)
    (1 + O(n u)) of the exact sum of the computed operands; the operands' own errors enter to first order plus their
    product."""
    sv, se = start
    acc = sv
    size = None if se is None else np.abs(sv)
    err = se
    for (av, ae), (bv, be) in terms:
        product = av * bv
        acc = acc - product if negate else acc + product
        if se is not None:
            size = size + np.abs(product)
            err = err + np.abs(av) * be + np.abs(bv) * ae + ae * be
    if se is not None:
        err = err + (len(terms) + 1) * UNIT * 1.01 * size
    return acc, err


def _times(x, y):
    (xv, xe), (yv, ye) = x, y
    value = xv * yv
    return value, None if xe is None else np.abs(xv) * ye + np.abs(yv) * xe + xe * ye + UNIT * np.abs(value)


def _sqrt(x):
    """sqrt to within one unit in the last place; an argument off by e moves it by at most e / (2 sqrt(x - e))."""
    xv, xe = x
    with np.errstate(invalid="ignore"):
        value = np.sqrt(xv)
        if xe is None:
            return value, None
        return value, xe / (2.0 * np.sqrt(np.maximum(xv - xe, 0.0))) + 2 * UNIT * np.abs(value)


def _reciprocal(x):
    xv, xe = x
    with np.errstate(divide="ignore", invalid="ignore"):
        value = 1.0 / xv
        if xe is None:
            return value, None
        return value, xe / (np.abs(xv) * (np.abs(xv) - xe)) + UNIT * np.abs(value)


def _log(x):
    """log to within two units in the last place of the result (a device's library logarithm), plus one unit of its
    argument's magnitude near 1 where the result is small; an argument off by e moves it by at most e / (x - e)."""
    xv, xe = x
    with np.errstate(divide="ignore", invalid="ignore"):
        value = np.log(xv)
        if xe is None:
            return value, None
        return value, xe / (xv - xe) + 2 * UNIT * np.abs(value) + UNIT


def _step(model, state, idx, uniforms, y, dtype, track):
    """The step on (value, error) pairs; `track` false: plain values (the errors are None)."""
    uniforms = np.asarray(uniforms, dtype=np.float64)
    B, K = uniforms.shape
    M, D = model["A"].shape[0], model["A"].shape[-1]
    Dy = model["C"].shape[-2]
    TD = D * (D + 1) // 2
    zero = np.zeros((B, K), dtype=dtype)
    given = lambda array: (np.asarray(array).astype(dtype), zero if track else None)
    flags = 0
    bad = np.zeros((B, K), dtype=bool)
    rows = np.arange(B)[:, None]
    if state is None:
        cdf_rows = np.broadcast_to(model["cdf0"], (B, K, M))
    else:
        regime_in, mean_in, cov_in = (np.asarray(part) for part in state)
        if idx is None:
            idx = np.broadcast_to(np.arange(K), (B, K))
        idx = np.asarray(idx)
        bad = (idx < 0) | (idx >= K)
        safe = np.where(bad, 0, idx)
        previous = regime_in[rows, safe]
        bad = bad | (previous < 0) | (previous >= M)
        previous = np.where(bad, 0, previous)
        cdf_rows = model["cdf"][previous]
        mean_in, cov_in = mean_in[rows, safe], cov_in[rows, safe]
    if bad.any():
        flags |= FLAG_INDEX_OUT_OF_RANGE
    s = (cdf_rows[:, :, :M - 1] <= uniforms[:, :, None]).sum(axis=2).astype(np.int32)
    A, bb, q, C, d, r = (model[name][s] for name in ("A", "b", "q", "C", "d", "r"))      # [B,K,...]
    y = np.asarray(y).astype(np.float64)

    # ---- predict
    if state is None:
        mp = [given(np.broadcast_to(model["m0"][i], (B, K))) for i in range(D)]
        Pm = {}
        for i in range(D):
            for j in range(i + 1):
                Pm[tri(i, j)] = given(np.broadcast_to(model["s0"][i] * model["s0"][i] if i == j else 0.0, (B, K)))
    else:
        m = [given(mean_in[:, :, i]) for i in range(D)]
        P = [given(cov_in[:, :, e]) for e in range(TD)]
        mp = [_chain(given(bb[:, :, i]), [(given(A[:, :, i, l]), m[l]) for l in range(D)]) for i in range(D)]
        W = [[_chain(given(zero), [(given(A[:, :, i, c]), P[tri(c, l)]) for c in range(D)]) for l in range(D)]
             for i in range(D)]
        Pm = {}
        for i in range(D):
            for j in range(i + 1):
                start = given(q[:, :, i] * q[:, :, i]) if i == j else given(zero)
                Pm[tri(i, j)] = _chain(start, [(given(A[:, :, i, l]), W[j][l]) for l in range(D)])
    # ---- innovation
    e = [_chain(given(y[:, None, i] - d[:, :, i]), [(given(C[:, :, i, l]), mp[l]) for l in range(D)], negate=True)
         for i in range(Dy)]
    U = [[_chain(given(zero), [(given(C[:, :, i, c]), Pm[tri(c, l)]) for c in range(D)]) for l in range(D)]
         for i in range(Dy)]
    S = {}
    for i in range(Dy):
        for j in range(i + 1):
            start = given(r[:, :, i] * r[:, :, i]) if i == j else given(zero)
            S[tri(i, j)] = _chain(start, [(given(C[:, :, i, l]), U[j][l]) for l in range(D)])
    # ---- the factor
    positive = np.ones((B, K), dtype=bool)
    rho, log_det = [], given(zero)
    for j in range(Dy):
        pivot = _chain(S[tri(j, j)], [(S[tri(j, c)], S[tri(j, c)]) for c in range(j)], negate=True)
        positive &= pivot[0] > 0
        S[tri(j, j)] = _sqrt(pivot)
        rho.append(_reciprocal(S[tri(j, j)]))
        log_det = _chain(log_det, [(_log(S[tri(j, j)]), given(zero + 1.0))])
        for i in range(j + 1, Dy):
            S[tri(i, j)] = _times(_chain(S[tri(i, j)], [(S[tri(i, c)], S[tri(j, c)]) for c in range(j)], negate=True),
                                  rho[j])
    # ---- the solves
    v, quad = [], given(zero)
    for i in range(Dy):
        v.append(_times(_chain(e[i], [(S[tri(i, c)], v[c]) for c in range(i)], negate=True), rho[i]))
        quad = _chain(quad, [(v[i], v[i])])
        for l in range(D):
            U[i][l] = _times(_chain(U[i][l], [(S[tri(i, c)], U[c][l]) for c in range(i)], negate=True), rho[i])
    # ---- outputs
    half = _chain(given(zero), [(given(zero - 0.5), quad)])
    log_w = _chain(_chain(half, [(log_det, given(zero + 1.0))], negate=True),
                   [(given(zero + Dy), given(zero + HALF_LOG_2PI))], negate=True)
    mean = [_chain(mp[l], [(U[i][l], v[i]) for i in range(Dy)]) for l in range(D)]
    cov = [_chain(Pm[tri(l, j)], [(U[i][l], U[i][j]) for i in range(Dy)], negate=True)
           for l in range(D) for j in range(l + 1)]
    dead = bad | ~positive

    def finish(parts):
        values = np.stack([part[0] for part in parts], axis=-1)
        values[dead] = np.nan
        errors = None
        if track:
            errors = np.stack([part[1] for part in parts], axis=-1).astype(np.float64)
            errors[dead] = 0.0
        return values, errors

    regime = np.where(bad, 0, s).astype(np.int32)
    (mean_v, mean_e), (cov_v, cov_e), (lw_v, lw_e) = finish(mean), finish(cov), finish([log_w])
    return (regime, mean_v, cov_v, lw_v[..., 0], flags), (mean_e, cov_e, None if lw_e is None else lw_e[..., 0])


def switching_kalman_step(model, state, idx, uniforms, y, dtype=np.float64):
    """(regime int32 [B,K], mean [B,K,D], cov [B,K,D(D+1)/2], log_weight [B,K], flags) of one step.

    model: `operands`' dict; state: None (the step-0 form: no input state, idx not read) or (regime int32 [B,K], mean
    [B,K,D], cov [B,K,D(D+1)/2]) — the stored particles of the step before; idx: int64 [B,K] or None (the identity);
    uniforms: float64 [B,K]; y: [B,Dy] of float32 or float64, widened; dtype: the arithmetic (np.float64: the contract;
    np.longdouble: what the bound is checked against).
    An idx outside [0, K) or a stored regime outside [0, M): regime 0, NaN mean, covariance and log-weight for that
    particle, FLAG_INDEX_OUT_OF_RANGE.  A pivot that is not positive: the drawn regime, NaN mean, covariance and
    log-weight (the resampling step that follows raises FLAG_NAN_LOG_WEIGHT)."""
    with np.errstate(all="ignore"):      # (an invalid particle's NaN travels through the arithmetic)
        return _step(model, state, idx, uniforms, y, dtype, False)[0]


def switching_kalman_step_bound(model, state, idx, uniforms, y):
    """(bound of mean [B,K,D], of cov [B,K,D(D+1)/2], of log_weight [B,K]), float64: how far a float64 evaluation of the
    step with fused multiply-adds (the kernel's) may lie from `switching_kalman_step`'s on the same inputs, derived and not
    measured.

    Every intermediate value carries a bound on its distance from the same expression in real arithmetic, pushed
    through the step operation by operation (a running error analysis), with u = 2^-53:

        a chain start + sum_{i<n} a_i b_i, fused or not:  sum_i (|a_i| db_i + |b_i| da_i + da_i db_i) + dstart
                                                          + 1.01 (n + 1) u (|start| + sum_i |a_i b_i|)
        x y:                |x| dy + |y| dx + dx dy + u |x y|
        sqrt(x):            dx / (2 sqrt(x - dx)) + 2 u sqrt(x)                 (the pivots: Lam_jj)
        1 / x:              dx / (|x| (|x| - dx)) + u / |x|                     (rho_j = 1 / Lam_jj)
        log(x):             dx / (x - dx) + 2 u |log x| + u                     (a library logarithm)

    so the two triangular solves amplify what reaches them by rho_i = 1 / Lam_ii at every row, as the arithmetic does.
    The model, the state, the observation and the uniforms enter exactly.  The bound returned is 2 * 1.01 times the
    running bound: two evaluations, each within it of the exact value.  Zero where the output is NaN."""
    with np.errstate(all="ignore"):
        _, (mean_e, cov_e, lw_e) = _step(model, state, idx, uniforms, y, np.float64, True)
    clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
    return clean(mean_e), clean(cov_e), clean(lw_e)


def _sensitivities(model, state, idx, regime, y):
    """How an error of the input state reaches a step's outputs, to first order, per step (the largest over the
    particles), from plain np.linalg on full matrices.  With G = I - K C, K = P- C^T S^-1 the gain and |.| the spectral
    norm (the Euclidean norm of a vector):

        dP- = A dP A^T,  dP = G dP- G^T                       |dP| <= |G|^2 |A|^2 |dP_in|
        dm  = G A dm_in + G dP- C^T S^-1 e                     |dm| <= |G| |A| |dm_in| + |G| |C^T S^-1 e| |A|^2 |dP_in|
        dlw = (S^-1 e)^T C A dm_in - 1/2 tr(C^T S^-1 C dP-) + 1/2 (C^T S^-1 e)^T dP- (C^T S^-1 e)
                                                               |dlw| <= |A^T C^T S^-1 e| |dm_in|
                                                                        + 1/2 (tr(C^T S^-1 C) + |C^T S^-1 e|^2) |A|^2 |dP_in|

    Returns (pp, mm, mp, wm, wp): the five factors above."""
    regime_in, mean_in, cov_in = state
    B, K = regime.shape
    D = mean_in.shape[-1]
    rows = np.arange(B)[:, None]
    if idx is not None:
        safe = np.clip(idx, 0, K - 1)
        mean_in, cov_in = mean_in[rows, safe], cov_in[rows, safe]
    A, C = model["A"][regime], model["C"][regime]
    Ct = np.swapaxes(C, -1, -2)
    predicted = A @ unpack(cov_in, D) @ np.swapaxes(A, -1, -2) + np.einsum("bki,ij->bkij", model["q"][regime] ** 2, np.eye(D))
    S = C @ predicted @ Ct + np.einsum("bki,ij->bkij", model["r"][regime] ** 2, np.eye(C.shape[-2]))
    good = np.isfinite(S).all(axis=(2, 3)) & np.isfinite(predicted).all(axis=(2, 3))
    S = np.where(good[:, :, None, None], S, np.eye(S.shape[-1]))
    predicted = np.where(good[:, :, None, None], predicted, 0.0)
    e = np.asarray(y, dtype=np.float64)[:, None, :] - np.einsum("bkij,bkj->bki", C, np.einsum(
        "bkij,bkj->bki", A, np.where(good[:, :, None], mean_in, 0.0)) + model["b"][regime]) - model["d"][regime]
    solved = np.linalg.solve(S, C)                                         # S^-1 C   [B,K,Dy,D]
    G = np.eye(D) - predicted @ Ct @ solved
    h = np.einsum("bkij,bki->bkj", solved, e)                              # C^T S^-1 e
    norm = lambda matrix: np.linalg.norm(matrix, 2, axis=(-2, -1))
    a, g = norm(A), norm(G)
    hn = np.linalg.norm(h, axis=-1)
    trace = np.einsum("bkij,bkij->bk", C, solved)
    return (float((g * g * a * a).max()), float((g * a).max()), float((g * hn * a * a).max()),
            float(np.linalg.norm(np.einsum("bkji,bkj->bki", A, h), axis=-1).max()),
            float((0.5 * (trace + hn * hn) * a * a).max()))


def switching_pass(observations, model, num_particles, regime_uniforms, resampling_uniforms):
    """The whole filter on replayed uniforms.  observations: T x [B,Dy]; model: `operands`' dict; regime_uniforms: T x
    float64 [B,K]; resampling_uniforms: (T-1) x [B] (systematic) or [B,K] (stratified).

    Returns a dict: log_marginal_likelihood [B] float64; regimes, means, covariances, log_weights (T arrays each: the stored,
    un-resampled particle systems); ancestral_indices ((T-1) x int64 [B,K]); flags; margins ((T-1) floats:
    `testing.adapted.ancestor_index`'s — only an index whose position lies this close to a step of the running sum of
    weights can differ on the device); and tolerances, propagated through the steps — how far a device run whose launches
    stay within their bounds (and whose ancestors and regimes are these) may lie from this one: `means`, `covariances`
    (T floats each: on the Euclidean norm of a particle's mean error and the spectral norm of its covariance error, which
    bound every element's), `log_weights` (T floats) and `log_marginal_likelihood` (one float).  With the factors of
    `_sensitivities`, the step's own bound in the Frobenius norm, and 1.01 for the terms of second order:

        tol_P[t]  = 1.01 pp tol_P[t-1] + max |cov bound|_F
        tol_m[t]  = 1.01 (mm tol_m[t-1] + mp tol_P[t-1]) + max |mean bound|_2
        tol_lw[t] = 1.01 (wm tol_m[t-1] + wp tol_P[t-1]) + max log-weight bound
        tol_Z    += tol_lw[t] + (K + 4) u (1 + max |lse| + log K)          (a log-sum-exp moves by at most its terms)."""
    T, K = len(observations), int(num_particles)
    out = {name: [] for name in ("regimes", "means", "covariances", "log_weights", "ancestral_indices", "margins")}
    tolerances = {"means": [], "covariances": [], "log_weights": []}
    state, idx, flags = None, None, 0
    log_z, tol_z = 0.0, 0.0
    for t in range(T):
        if t > 0:
            idx, lse, bits, margin = _adapted.ancestor_index(out["log_weights"][-1], resampling_uniforms[t - 1])
            flags |= bits
            out["ancestral_indices"].append(idx), out["margins"].append(margin)
            log_z = log_z + lse - np.log(K)
            tol_z += tolerances["log_weights"][-1] + (K + 4) * UNIT * (1.0 + float(np.abs(lse).max()) + np.log(K))
        regime, mean, cov, log_w, bits = switching_kalman_step(model, state, idx, regime_uniforms[t], observations[t])
        bound_m, bound_p, bound_w = switching_kalman_step_bound(model, state, idx, regime_uniforms[t], observations[t])
        D = mean.shape[-1]
        fresh_m = float(np.sqrt((bound_m ** 2).sum(axis=-1)).max())
        fresh_p = float(np.sqrt((unpack(bound_p, D) ** 2).sum(axis=(-2, -1))).max())
        fresh_w = float(bound_w.max())
        if t == 0:
            tol_m, tol_p, tol_w = fresh_m, fresh_p, fresh_w
        else:
            pp, mm, mp, wm, wp = _sensitivities(model, state, idx, regime, observations[t])
            before_m, before_p = tolerances["means"][-1], tolerances["covariances"][-1]
            tol_p = 1.01 * pp * before_p + fresh_p
            tol_m = 1.01 * (mm * before_m + mp * before_p) + fresh_m
            tol_w = 1.01 * (wm * before_m + wp * before_p) + fresh_w
        flags |= bits
        state = (regime, mean, cov)
        tolerances["means"].append(tol_m), tolerances["covariances"].append(tol_p), tolerances["log_weights"].append(tol_w)
        out["regimes"].append(regime), out["means"].append(mean), out["covariances"].append(cov)
        out["log_weights"].append(log_w)
    with np.errstate(invalid="ignore"):
        top = out["log_weights"][-1].max(axis=1)
        lse = top + np.log(np.exp(out["log_weights"][-1] - top[:, None]).sum(axis=1))
    log_z = log_z + lse - np.log(K)
    tol_z += tolerances["log_weights"][-1] + (K + 4) * UNIT * (1.0 + float(np.abs(lse).max()) + np.log(K))
    tolerances["log_marginal_likelihood"] = float(tol_z)
    out.update(log_marginal_likelihood=log_z, flags=flags, tolerances=tolerances)
    return out


def moments(regimes, means, covariances, log_weights, num_regimes):
    """(filtered_mean [T,B,D], filtered_covariance [T,B,D,D], regime_probabilities [T,B,M]) of a pass's stored particle
    systems: the mixture's moments, sum_k w_k (P_k + m_k m_k^T) - mean mean^T, with w = softmax(log_weight)."""
    fm, fc, rp = [], [], []
    for regime, mean, cov, log_w in zip(regimes, means, covariances, log_weights):
        w = np.exp(log_w - log_w.max(axis=1, keepdims=True))
        w = w / w.sum(axis=1, keepdims=True)
        D = mean.shape[-1]
        average = (w[:, :, None] * mean).sum(axis=1)
        second = (w[:, :, None, None] * (unpack(cov, D) + mean[:, :, :, None] * mean[:, :, None, :])).sum(axis=1)
        fm.append(average), fc.append(second - average[:, :, None] * average[:, None, :])
        rp.append(np.stack([(w * (regime == i)).sum(axis=1) for i in range(num_regimes)], axis=1))
    return np.stack(fm), np.stack(fc), np.stack(rp)


def exact_log_likelihood(model, ys):
    """log p(y_0..y_{T-1}) [B] by enumerating all M^T regime sequences, each an exact Kalman filter (plain np.linalg on
    full matrices).  ys: T x [B,Dy] (or T x [Dy]: one series, a scalar back)."""
    ys = [np.asarray(y, dtype=np.float64) for y in ys]
    single = ys[0].ndim == 1
    if single:
        ys = [y[None, :] for y in ys]
    T, B = len(ys), ys[0].shape[0]
    M, D = model["A"].shape[0], model["A"].shape[-1]
    Dy = model["C"].shape[-2]
    terms = []
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    for sequence in itertools.product(range(M), repeat=T):
        total = np.full(B, log_pi0[sequence[0]])
        mean = np.broadcast_to(model["m0"], (B, D)).copy()
        cov = np.diag(model["s0"] ** 2)
        for t, s in enumerate(sequence):
            A, C = model["A"][s], model["C"][s]
            if t > 0:
                total = total + log_Pi[sequence[t - 1], s]
                mean, cov = mean @ A.T + model["b"][s], A @ cov @ A.T + np.diag(model["q"][s] ** 2)
            S = C @ cov @ C.T + np.diag(model["r"][s] ** 2)
            residual = ys[t] - mean @ C.T - model["d"][s]
            solved = np.linalg.solve(S, residual.T).T
            total = total - 0.5 * ((residual * solved).sum(axis=1) + np.linalg.slogdet(S)[1] + 2 * Dy * HALF_LOG_2PI)
            gain = cov @ C.T @ np.linalg.inv(S)
            mean, cov = mean + residual @ gain.T, cov - gain @ C @ cov
        terms.append(total)
    terms = np.stack(terms)
    top = terms.max(axis=0)
    out = top + np.log(np.exp(terms - top).sum(axis=0))
    return out[0] if single else out


# ---- the inputs the tests and the benchmark share -------------------------------------------------------------------------------
# (B, K, M, D, Dy): one lane; a partial wavefront; a 256-particle tile that straddles batch rows; several workgroups; every
# padded extent of the kernel (2, 4, 8 for D and for Dy); the largest M
STEP_SHAPES = [(1, 1, 1, 1, 1), (3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3), (1, 257, 16, 8, 1), (2, 1025, 2, 3, 2)]


def example_model(M, D, Dy, seed=0):
    """`operands` of a well-conditioned model: A orthogonal scaled by 0.5 .. 0.8, q and r in [0.3, 0.8], C = I + 0.3 N."""
    rng = np.random.default_rng([seed, M, D, Dy])
    A = np.stack([np.linalg.qr(rng.standard_normal((D, D)))[0] * rng.uniform(0.5, 0.8) for _ in range(M)])
    C = np.stack([np.eye(Dy, D) + 0.3 * rng.standard_normal((Dy, D)) for _ in range(M)])
    Pi = rng.uniform(0.2, 1.0, (M, M))
    pi0 = rng.uniform(0.2, 1.0, M)
    return operands(pi0 / pi0.sum(), Pi / Pi.sum(axis=1, keepdims=True), rng.standard_normal(D), rng.uniform(0.5, 1.5, D),
                    A, 0.3 * rng.standard_normal((M, D)), rng.uniform(0.3, 0.8, (M, D)), C,
                    0.3 * rng.standard_normal((M, Dy)), rng.uniform(0.3, 0.8, (M, Dy)))


def example_step(B, K, M, D, Dy, index="none", later=True, observation_dtype=np.float64, seed=0):
    """(model, state, idx, uniforms, y) of one step: `later` false — the step-0 form (state and idx None); index 'none',
    'sorted' or 'unsorted'.  The state is a random regime, a standard-normal mean and a covariance F F^T / D + 0.1 I."""
    rng = np.random.default_rng([seed, B, K, M, D, Dy])
    model = example_model(M, D, Dy, seed)
    uniforms = rng.uniform(size=(B, K))
    y = rng.standard_normal((B, Dy)).astype(observation_dtype)
    if not later:
        return model, None, None, uniforms, y
    factor = rng.standard_normal((B, K, D, D))
    cov = pack(factor @ np.swapaxes(factor, -1, -2) / D + 0.1 * np.eye(D))
    state = (rng.integers(0, M, (B, K)).astype(np.int32), rng.standard_normal((B, K, D)), np.ascontiguousarray(cov))
    idx = None
    if index != "none":
        idx = rng.integers(0, K, (B, K)).astype(np.int64)
        if index == "sorted":
            idx = np.sort(idx, axis=1)
    return model, state, idx, uniforms, y
