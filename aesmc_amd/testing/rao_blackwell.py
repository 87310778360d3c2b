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


# ---- the fully adapted filter: the look-ahead (K32), the draw (K33) and the pass they make -----------------------------------------
# The regimes are drawn from their exact posterior (Chen & Liu 2000; Doucet, Gordon & Krishnamurthy 2001; the fully adapted
# auxiliary particle filter of Pitt & Shephard 1999).  For the STORED particle (s, m, P) and every regime j, with l_j the
# step's log-likelihood under s_t = j (everything above up to `log w`, the draw replaced by j, no ancestors):
#
#     g_j     = log_prior[s, j] + l_j (step 0: log_prior[j]); -inf where the log-prior is -inf WHATEVER l_j is (a pivot that
#               is not positive there is ignored); NaN where the log-prior is finite and a pivot is not positive
#     log w   = top + log(0 + sum_j exp(g_j - top)),  top = max_j g_j
#     cdf_j   = 0 + sum_{i <= j} exp(g_i - log w); exactly 1 from the last i with exp(g_i - log w) > 0 onwards
#
# and the draw is the step with s = #{ i < M-1 : cdf[b,a,i] <= uniforms[b,k] } for the ancestor a.
def _forced(model, regime):
    """(model, uniforms) under which `_step` draws exactly `regime` [B,K] for every particle whatever its ancestor: every
    cumulative row replaced by (1/M, 2/M, .., 1) and the uniform by (regime + 1/2) / M.  Nothing else of the step changes."""
    M = model["A"].shape[0]
    edges = (np.arange(M) + 1.0) / M
    shim = dict(model, cdf0=edges, cdf=np.ascontiguousarray(np.broadcast_to(edges, (M, M))))
    return shim, (np.asarray(regime, dtype=np.float64) + 0.5) / M


def _exp(x):
    """exp to within two units in the last place (a device's library exponential); an argument off by e moves it by at most
    exp(x) (exp(e) - 1)."""
    xv, xe = x
    value = np.exp(xv)
    if xe is None:
        return value, None
    return value, value * np.expm1(xe) + 2 * UNIT * value


def _minus(x, y):
    """x - y, one rounding; exact (and -inf) where x is -inf."""
    (xv, xe), (yv, ye) = x, y
    value = xv - yv
    if xe is None:
        return value, None
    return value, np.where(np.isneginf(value), 0.0, xe + ye + UNIT * np.abs(value))


def _lookahead(model, log_prior, state, y, num_particles, dtype, track):
    y = np.asarray(y)
    B, M = y.shape[0], model["A"].shape[0]
    K = int(num_particles) if state is None else np.asarray(state[0]).shape[1]
    log_prior = np.asarray(log_prior, dtype=np.float64)
    zero = np.zeros((B, K), dtype=dtype)
    given = lambda array: (np.asarray(array).astype(dtype), zero if track else None)
    one = given(zero + 1.0)
    bad = np.zeros((B, K), dtype=bool)
    if state is None:
        prior = np.broadcast_to(log_prior, (B, K, M))
    else:
        previous = np.asarray(state[0])
        bad = (previous < 0) | (previous >= M)
        prior = log_prior[np.where(bad, 0, previous)]
    flags, scores = 0, []
    for j in range(M):
        shim, forced = _forced(model, np.full((B, K), j))
        (_, _, _, ell, bits), (_, _, ell_e) = _step(shim, state, None, forced, y, dtype, track)
        flags |= bits
        excluded = np.isneginf(prior[:, :, j])
        value, error = _chain(given(np.where(excluded, 0.0, prior[:, :, j])), [((ell, ell_e), one)])
        value = np.where(excluded & ~bad, -np.inf, value)
        scores.append((value, np.where(excluded, 0.0, error) if track else None))
    top = scores[0][0]
    for value, _ in scores[1:]:
        top = np.maximum(top, value)      # (a NaN stays)
    top = (top, np.maximum.reduce([error for _, error in scores]) if track else None)
    total = _chain(given(zero), [(_exp(_minus(score, top)), one) for score in scores])
    log_w = _chain(top, [(_log(total), one)])
    terms = [_exp(_minus(score, log_w)) for score in scores]
    running, rows = given(zero), []
    for term in terms:
        running = _chain(running, [(term, one)])
        rows.append(running)
    positive = np.stack([term[0] > 0 for term in terms], axis=-1)
    last = M - 1 - np.argmax(positive[:, :, ::-1], axis=-1)
    forced_one = np.arange(M)[None, None, :] >= last[:, :, None]
    invalid = np.isnan(log_w[0])
    cdf = np.stack([row[0] for row in rows], axis=-1)
    cdf_e = None
    if track:      # (where both sides set the entry to 1 the distance is 0; where they disagree on `last`, this)
        cdf_e = np.stack([row[1] for row in rows], axis=-1).astype(np.float64)
        cdf_e = np.where(forced_one, cdf_e + np.abs(1.0 - cdf).astype(np.float64), cdf_e)
        cdf_e[invalid] = 0.0
    cdf = np.where(forced_one, 1.0, cdf).astype(dtype)
    cdf[invalid] = np.nan
    return (log_w[0], cdf, flags), (np.where(invalid, 0.0, log_w[1]).astype(np.float64) if track else None, cdf_e)


def switching_lookahead(model, log_prior, state, y, num_particles=None, dtype=np.float64):
    """(log_weight [B,K], cdf [B,K,M], flags) of one look-ahead (include/aesmc_hip.h: aesmc_switching_lookahead, K32).

    model: `operands`' dict (cdf0 and cdf are not read); log_prior: float64 [M,M] with a state (rows: from-regime), [M]
    without one — the logarithms of Pi or pi0, -inf where a probability is 0; state: None (step 0: every regime predicted by
    m0 and diag(s0^2); `num_particles` gives K) or the stored (regime, mean, cov); y [B,Dy]; dtype: the arithmetic.
    A stored regime outside [0, M): NaN log-weight and NaN CDF row, FLAG_INDEX_OUT_OF_RANGE.  A pivot that is not positive
    under a regime of finite log-prior, or no regime of finite log-prior: NaN log-weight and NaN CDF row."""
    with np.errstate(all="ignore"):
        return _lookahead(model, log_prior, state, y, num_particles, dtype, False)[0]


def switching_lookahead_bound(model, log_prior, state, y, num_particles=None):
    """(bound of log_weight [B,K], of cdf [B,K,M]), float64: `switching_kalman_step_bound`'s running analysis carried on
    through the scores (one addition), the log-sum-exp, the exponentials and the cumulative sum, with

        exp(x):   exp(x) (exp(dx) - 1) + 2 u exp(x)                (a library exponential)
        x - y:    dx + dy + u |x - y|                               (exact where x is -inf)
        max_j:    the largest of the scores' bounds

    and 2 * 1.01 times the running bound returned, as there.  Zero where the output is NaN."""
    with np.errstate(all="ignore"):
        _, (lw_e, cdf_e) = _lookahead(model, log_prior, state, y, num_particles, np.float64, True)
    clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
    return clean(lw_e), clean(cdf_e)


def _draw(model, state, idx, uniforms, cdf, y, dtype, track):
    uniforms = np.asarray(uniforms, dtype=np.float64)
    B, K = uniforms.shape
    M = model["A"].shape[0]
    rows = np.asarray(cdf, dtype=np.float64)
    if state is not None and idx is not None:
        idx = np.asarray(idx)
        rows = rows[np.arange(B)[:, None], np.where((idx < 0) | (idx >= K), 0, idx)]
    s = (rows[:, :, :M - 1] <= uniforms[:, :, None]).sum(axis=2)      # (a NaN row: regime 0)
    shim, forced = _forced(model, s)
    return _step(shim, state, idx, forced, y, dtype, track), rows


def switching_kalman_draw(model, state, idx, uniforms, cdf, y, dtype=np.float64):
    """(regime int32 [B,K], mean, cov, log_likelihood [B,K], flags): `switching_kalman_step` with the regime drawn from the
    ancestor's row of `cdf` [B,K,M] (include/aesmc_hip.h: aesmc_switching_kalman_draw, K33) — `_step` itself under
    `_forced`.  Everything else, the conventions included, as `switching_kalman_step`."""
    with np.errstate(all="ignore"):
        return _draw(model, state, idx, uniforms, cdf, y, dtype, False)[0][0]


def switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y):
    """`switching_kalman_step_bound` of the draw: (bound of mean, of cov, of log_likelihood)."""
    with np.errstate(all="ignore"):
        (_, (mean_e, cov_e, ll_e)), _ = _draw(model, state, idx, uniforms, cdf, y, np.float64, True)
    clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
    return clean(mean_e), clean(cov_e), clean(ll_e)


def score_from_cdf(log_weight, cdf, regime, bound_w=None, bound_c=None):
    """(g_s [B,K], its bound or None): the score of regime `regime[b,k]` recovered from a look-ahead's outputs,
    g_s = log(cdf_s - cdf_{s-1}) + log_weight (cdf_{-1} = 0).  With the look-ahead's bounds, how far the value recovered from
    outputs within them may lie from the one recovered here: the difference d carries both entries' bounds, the logarithm
    divides by d less that — infinite where nothing of d is left."""
    B, K, _ = cdf.shape
    rows, cols = np.arange(B)[:, None], np.arange(K)[None, :]
    regime = np.asarray(regime).astype(np.int64)
    below = np.where(regime > 0, cdf[rows, cols, np.maximum(regime - 1, 0)], 0.0)
    d = cdf[rows, cols, regime] - below
    with np.errstate(all="ignore"):
        value = np.log(d) + log_weight
        if bound_w is None:
            return value, None
        error = bound_c[rows, cols, regime] + np.where(regime > 0, bound_c[rows, cols, np.maximum(regime - 1, 0)], 0.0) + UNIT * d
        bound = np.where(d > 2 * error, error / (d - error), np.inf) + 2 * UNIT * np.abs(np.log(d)) + UNIT + bound_w + \
            UNIT * np.abs(value)
    return value, 2 * 1.01 * bound


def _regime_margin(rows, uniforms):
    """The smallest |cdf[b,a,i] - u[b,k]| over i < M-1: only a regime whose uniform lies this close to an entry of its row
    can differ on the device.  An entry that is exactly 1 (set, not summed, on both sides) is above every uniform."""
    edges = rows[:, :, :rows.shape[-1] - 1]
    with np.errstate(invalid="ignore"):
        distance = np.where(edges < 1.0, np.abs(edges - np.asarray(uniforms)[:, :, None]), np.inf)
    return float(distance.min()) if distance.size else float("inf")


def adapted_switching_pass(observations, model, num_particles, regime_uniforms, resampling_uniforms):
    """The fully adapted filter on replayed uniforms: at every step the look-ahead on the stored system of the step before
    (step 0: on the prior), the resampling on ITS log-weights (step 0: none), and the draw through the ancestors.  Arguments
    as `switching_pass`.

    Returns a dict: log_marginal_likelihood [B] float64 (the sum of the row log-sum-exps of the first-stage log-weights minus
    log K each); regimes, means, covariances (T arrays each: the stored, equally weighted systems after the draw);
    log_likelihoods (T x [B,K]: l_s of the draw, which the filter does not use); first_stage_log_weights (T x [B,K]);
    ancestral_indices ((T-1) x int64 [B,K]); flags; margins: {"resampling": (T-1) floats, `ancestor_index`'s;
    "regimes": T floats, the smallest distance of a regime uniform from an entry (below 1) of its posterior row}; and
    tolerances, propagated as `switching_pass` propagates its own, with the factors of `_sensitivities`:

        tol_P[t], tol_m[t]   as there, from the draw's bound
        tol_g[t]  = 1.01 max_j (wm_j tol_m[t-1] + wp_j tol_P[t-1])       (what the input state's error does to a score; over
                                                                         the regimes of positive prior probability)
        tol_lw[t] = tol_g[t] + max log-weight bound       (`first_stage_log_weights`: a log-sum-exp moves by at most its terms)
        tol_c[t]  = tol_g[t] + max cdf bound              (`cdf`: sum_l |d cdf_j / d g_l| = 2 cdf_j (1 - cdf_j) <= 1/2)
        tol_Z    += tol_lw[t] + (K + 4) u (1 + max |lse| + log K)."""
    T, K = len(observations), int(num_particles)
    M = model["A"].shape[0]
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    out = {name: [] for name in ("regimes", "means", "covariances", "log_likelihoods", "first_stage_log_weights",
                                 "ancestral_indices")}
    margins = {"resampling": [], "regimes": []}
    tolerances = {name: [] for name in ("means", "covariances", "log_likelihoods", "first_stage_log_weights", "cdf")}
    state, flags = None, 0
    log_z, tol_z = 0.0, 0.0
    for t in range(T):
        y = observations[t]
        B = np.asarray(y).shape[0]
        prior = log_pi0 if t == 0 else log_Pi
        log_w, cdf, bits = switching_lookahead(model, prior, state, y, K)
        bound_w, bound_c = switching_lookahead_bound(model, prior, state, y, K)
        flags |= bits
        carried = 0.0
        if t > 0:
            before_m, before_p = tolerances["means"][-1], tolerances["covariances"][-1]
            rows = log_Pi[np.clip(state[0], 0, M - 1)]
            for j in range(M):      # (a particle for which regime j is excluded stands in with its likeliest successor)
                considered = np.where(np.isneginf(rows[:, :, j]), np.argmax(rows, axis=-1), j)
                _, _, _, wm, wp = _sensitivities(model, state, None, considered, y)
                carried = max(carried, 1.01 * (wm * before_m + wp * before_p))
        tolerances["first_stage_log_weights"].append(carried + float(bound_w.max()))
        tolerances["cdf"].append(carried + float(bound_c.max()))
        if t == 0:
            idx = None
            with np.errstate(invalid="ignore"):
                top = log_w.max(axis=1)
                lse = top + np.log(np.exp(log_w - top[:, None]).sum(axis=1))
        else:
            idx, lse, bits, margin = _adapted.ancestor_index(log_w, resampling_uniforms[t - 1])
            flags |= bits
            out["ancestral_indices"].append(idx), margins["resampling"].append(margin)
        log_z = log_z + lse - np.log(K)
        tol_z += tolerances["first_stage_log_weights"][-1] + (K + 4) * UNIT * (1.0 + float(np.abs(lse).max()) + np.log(K))
        with np.errstate(all="ignore"):
            ((regime, mean, cov, ell, bits), _), rows = _draw(model, state, idx, regime_uniforms[t], cdf, y, np.float64, False)
        bound_m, bound_p, bound_l = switching_kalman_draw_bound(model, state, idx, regime_uniforms[t], cdf, y)
        flags |= bits
        margins["regimes"].append(_regime_margin(rows, regime_uniforms[t]))
        D = mean.shape[-1]
        fresh_m = float(np.sqrt((bound_m ** 2).sum(axis=-1)).max())
        fresh_p = float(np.sqrt((unpack(bound_p, D) ** 2).sum(axis=(-2, -1))).max())
        fresh_l = float(bound_l.max())
        if t == 0:
            tol_m, tol_p, tol_l = fresh_m, fresh_p, fresh_l
        else:
            pp, mm, mp, wm, wp = _sensitivities(model, state, idx, regime, y)
            tol_p = 1.01 * pp * before_p + fresh_p
            tol_m = 1.01 * (mm * before_m + mp * before_p) + fresh_m
            tol_l = 1.01 * (wm * before_m + wp * before_p) + fresh_l
        state = (regime, mean, cov)
        tolerances["means"].append(tol_m), tolerances["covariances"].append(tol_p), tolerances["log_likelihoods"].append(tol_l)
        out["regimes"].append(regime), out["means"].append(mean), out["covariances"].append(cov)
        out["log_likelihoods"].append(ell), out["first_stage_log_weights"].append(log_w)
    tolerances["log_marginal_likelihood"] = float(tol_z)
    out.update(log_marginal_likelihood=log_z, flags=flags, tolerances=tolerances, margins=margins)
    return out


def sticky_example(T=12, seed=0):
    """(model, one series: T x [Dy]) where a look-ahead pays: three sticky regimes (0.96 on the diagonal) with
    well-separated emission offsets (-4, 0, 4 against r = 0.5) over a slowly moving scalar state — a regime change shows in
    the observation at once, and a bootstrap on the regimes finds it only with the particles that guessed it.  The series
    is simulated from the model (a fixed generator)."""
    M, D, Dy = 3, 1, 1
    Pi = np.full((M, M), 0.02) + 0.94 * np.eye(M)
    model = operands(np.full(M, 1.0 / M), Pi, np.zeros(D), np.ones(D), np.full((1, D, D), 0.9), np.zeros((1, D)),
                     np.full((1, D), 0.3), np.ones((1, Dy, D)), np.array([[-4.0], [0.0], [4.0]]), np.full((1, Dy), 0.5))
    rng = np.random.default_rng([seed, 1999])
    series, s, z = [], None, None
    for t in range(T):
        s = rng.choice(M, p=model["pi0"] if t == 0 else model["Pi"][s])
        z = model["m0"] + model["s0"] * rng.standard_normal(D) if t == 0 else \
            model["A"][s] @ z + model["b"][s] + model["q"][s] * rng.standard_normal(D)
        series.append(model["C"][s] @ z + model["d"][s] + model["r"][s] * rng.standard_normal(Dy))
    return model, series


# ---- Rao-Blackwellised backward simulation: the information step (K34), the pair scores (K35) and the pass they make -----------
# Fong, Godsill, Doucet & West 2002; Whiteley, Andrieu & Doucet 2010; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016.  Once
# z is integrated out the regimes are not Markov: a trajectory carries backwards, for its future regimes s'_{t+1..T-1},
#
#     p(y_{t+1..T-1} | z_t, s'_{t+1..T-1}) = exp(c_t + lam_t^T z_t - 1/2 z_t^T Om_t z_t),     Om_{T-1} = 0, lam_{T-1} = 0, c_{T-1} = 0
#
# and every stored particle (s, m, P, log w) of step t is scored by the closed-form integral of that against N(m, P).
#
# The information step, per trajectory, with j = s'_{t+1}, y = y_{t+1}, r2_i = r_j[i]^2, q2_i = q_j[i]^2, sq_i = sqrt(q2_i) (every
# sum in ascending index order from the value named first; symmetric matrices as packed lower triangles, `tri`):
#
#     e_i    = y_i - d_j[i];  rho_i = 1 / r2_i;  G_il = C_j[i,l] rho_i
#     Oh_ab  = Om_ab + sum_i G_ia C_j[i,b];   lh_a = lam_a + sum_i G_ia e_i
#     ch     = ((c - 1/2 sum_i (e_i rho_i) e_i) - 1/2 sum_i log r2_i) - Dy (1/2 log 2 pi)
#     Mm_ab  = (a == b) + (sq_a sq_b) Oh_ab;  L = chol(Mm) column by column as K31's (the pivots are at least 1)
#     X      = L^-1 (diag(sq) Oh),  w = L^-1 (diag(sq) lh)       (forward substitutions, one reciprocal per pivot)
#     Ot_ab  = Oh_ab - sum_i X_ia X_ib;   g_a = lh_a - sum_i X_ia w_i
#     ob_a   = sum_l Ot_al b_j[l];  Om'_ab = sum_i A_j[i,a] (sum_c Ot_ic A_j[c,b]);  lam'_a = sum_i A_j[i,a] (g_i - ob_i)
#     c'     = (((ch - sum_i log L_ii) + 1/2 sum_i w_i^2) + sum_i b_j[i] g_i) - sum_i (1/2 b_j[i]) ob_i
#     F      = the lower factor of Om' (F F^T = Om', Phi = F^T), column by column; with tau = 2^-40 max_i Om'_ii:
#              p_k = Om'_kk - sum_{c<k} F_kc^2;  p_k <= tau: column k of F is zero;  otherwise F_kk = sqrt(p_k),
#              F_ik = (Om'_ik - sum_{c<k} F_ic F_kc) / F_kk       (Om' is only positive SEMI-definite: rank <= Dy at t = T-2)
#
# The pair score of trajectory n and particle k, reading only F and lam' (Om' m = F (F^T m)):
#
#     t_i = sum_{l>=i} F_li m_l;  mq = sum_i t_i^2;  h_l = lam'_l - sum_{i<=l} F_li t_i;  lm = sum_l lam'_l m_l
#     hph = sum_c h_c (sum_l P_cl h_l)
#     W_il = sum_{c>=i} F_ci P_cl;  v_i = sum_l W_il h_l;  Lam_ij = (i == j) + sum_{l>=j} W_il F_lj   (j <= i; pivots at least 1)
#     G = chol(Lam);  x = G^-1 v;  xq = sum_i x_i^2;  ld = sum_i log G_ii
#     score = ((((log w + log Pi[s, s']) + lm) - 1/2 mq) + 1/2 (hph - xq)) - ld;     -inf where log Pi[s, s'] is -inf
def _information(model, regime_next, info, y, dtype, track):
    regime_next = np.asarray(regime_next)
    B, N = regime_next.shape
    M, D = model["A"].shape[0], model["A"].shape[-1]
    Dy = model["C"].shape[-2]
    TD = D * (D + 1) // 2
    zero = np.zeros((B, N), dtype=dtype)
    given = lambda array: (np.asarray(array).astype(dtype), zero if track else None)
    one = given(zero + 1.0)
    bad = (regime_next < 0) | (regime_next >= M)
    flags = FLAG_INDEX_OUT_OF_RANGE if bad.any() else 0
    j = np.where(bad, 0, regime_next)
    A, bb, q, C, d, r = (model[name][j] for name in ("A", "b", "q", "C", "d", "r"))      # [B,N,...]
    y = np.asarray(y).astype(np.float64)
    if info is None:
        Om, lam, c = [given(zero)] * TD, [given(zero)] * D, given(zero)
    else:
        omega_in, lambda_in, c_in = (np.asarray(part) for part in info)
        Om = [given(omega_in[:, :, e]) for e in range(TD)]
        lam = [given(lambda_in[:, :, i]) for i in range(D)]
        c = given(c_in)
    Cm = [[given(C[:, :, i, l]) for l in range(D)] for i in range(Dy)]
    Am = [[given(A[:, :, i, l]) for l in range(D)] for i in range(D)]
    bv = [given(bb[:, :, i]) for i in range(D)]
    # ---- the observation
    e = [given(y[:, None, i] - d[:, :, i]) for i in range(Dy)]
    r2 = [given(r[:, :, i] * r[:, :, i]) for i in range(Dy)]
    rho = [_reciprocal(x) for x in r2]
    G = [[_times(Cm[i][l], rho[i]) for l in range(D)] for i in range(Dy)]
    Oh = [_chain(Om[tri(a, b)], [(G[i][a], Cm[i][b]) for i in range(Dy)]) for a in range(D) for b in range(a + 1)]
    lh = [_chain(lam[a], [(G[i][a], e[i]) for i in range(Dy)]) for a in range(D)]
    quad = _chain(given(zero), [(_times(e[i], rho[i]), e[i]) for i in range(Dy)])
    logr = _chain(given(zero), [(_log(r2[i]), one) for i in range(Dy)])
    ch = _chain(_chain(_chain(c, [(given(zero - 0.5), quad)]), [(given(zero - 0.5), logr)]),
                [(given(zero + Dy), given(zero + HALF_LOG_2PI))], negate=True)
    # ---- the transition's noise integrated out
    # (the root of an exact argument, which may be zero: two units in its last place, as `_sqrt`'s own rounding term)
    sq = [(value, 2 * UNIT * value if track else None)
          for value in (np.sqrt((q[:, :, i] * q[:, :, i]).astype(dtype)) for i in range(D))]
    Mm = {}
    for a in range(D):
        for b in range(a + 1):
            Mm[tri(a, b)] = _chain(given(zero + (1.0 if a == b else 0.0)), [(_times(sq[a], sq[b]), Oh[tri(a, b)])])
    inv, log_det = [], given(zero)
    for k in range(D):
        pivot = _chain(Mm[tri(k, k)], [(Mm[tri(k, c)], Mm[tri(k, c)]) for c in range(k)], negate=True)
        Mm[tri(k, k)] = _sqrt(pivot)
        inv.append(_reciprocal(Mm[tri(k, k)]))
        log_det = _chain(log_det, [(_log(Mm[tri(k, k)]), one)])
        for i in range(k + 1, D):
            Mm[tri(i, k)] = _times(_chain(Mm[tri(i, k)], [(Mm[tri(i, c)], Mm[tri(k, c)]) for c in range(k)], negate=True),
                                   inv[k])
    X, w = [], []
    for i in range(D):
        X.append([_times(_chain(_times(sq[i], Oh[tri(i, l)]), [(Mm[tri(i, c)], X[c][l]) for c in range(i)], negate=True),
                         inv[i]) for l in range(D)])
        w.append(_times(_chain(_times(sq[i], lh[i]), [(Mm[tri(i, c)], w[c]) for c in range(i)], negate=True), inv[i]))
    Ot = [_chain(Oh[tri(a, b)], [(X[i][a], X[i][b]) for i in range(D)], negate=True) for a in range(D) for b in range(a + 1)]
    g = [_chain(lh[a], [(X[i][a], w[i]) for i in range(D)], negate=True) for a in range(D)]
    ww = _chain(given(zero), [(w[i], w[i]) for i in range(D)])
    # ---- back through the transition
    ob = [_chain(given(zero), [(Ot[tri(a, l)], bv[l]) for l in range(D)]) for a in range(D)]
    gb = [_chain(g[a], [(ob[a], one)], negate=True) for a in range(D)]
    Wt = [[_chain(given(zero), [(Ot[tri(i, c)], Am[c][b]) for c in range(D)]) for b in range(D)] for i in range(D)]
    Om_out = [_chain(given(zero), [(Am[i][a], Wt[i][b]) for i in range(D)]) for a in range(D) for b in range(a + 1)]
    lam_out = [_chain(given(zero), [(Am[i][a], gb[i]) for i in range(D)]) for a in range(D)]
    c_out = _chain(_chain(_chain(_chain(ch, [(log_det, one)], negate=True), [(given(zero + 0.5), ww)]),
                          [(bv[i], g[i]) for i in range(D)]),
                   [(given(0.5 * bb[:, :, i]), ob[i]) for i in range(D)], negate=True)
    # ---- the factor of a matrix that is only positive semi-definite
    F = {e_: Om_out[e_] for e_ in range(TD)}
    top = Om_out[0][0]
    for i in range(1, D):
        top = np.maximum(top, Om_out[tri(i, i)][0])
    tau = top * dtype(2.0 ** -40)
    margin = np.full((B, N), np.inf)
    for k in range(D):
        pivot = _chain(F[tri(k, k)], [(F[tri(k, c)], F[tri(k, c)]) for c in range(k)], negate=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            keep = pivot[0] > tau
            margin = np.minimum(margin, np.where(top > 0, np.abs((pivot[0] - tau).astype(np.float64)) /
                                                 np.maximum(top.astype(np.float64), 1e-300), np.inf))
        safe = (np.where(keep, pivot[0], 1.0), None if not track else np.where(keep, pivot[1], 0.0))
        root = _sqrt(safe)
        rk = _reciprocal(root)
        F[tri(k, k)] = (np.where(keep, root[0], 0.0), None if not track else np.where(keep, root[1], 0.0))
        for i in range(k + 1, D):
            value = _times(_chain(F[tri(i, k)], [(F[tri(i, c)], F[tri(k, c)]) for c in range(k)], negate=True), rk)
            F[tri(i, k)] = (np.where(keep, value[0], 0.0), None if not track else np.where(keep, value[1], 0.0))

    def finish(parts):
        values = np.stack([part[0] for part in parts], axis=-1)
        values[bad] = np.nan
        errors = None
        if track:
            errors = np.stack([part[1] for part in parts], axis=-1).astype(np.float64)
            errors[bad] = 0.0
        return values, errors

    (om_v, om_e), (lam_v, lam_e), (c_v, c_e), (f_v, f_e) = finish(Om_out), finish(lam_out), finish([c_out]), \
        finish([F[e_] for e_ in range(TD)])
    margin = np.where(bad, np.inf, margin)
    return (om_v, lam_v, c_v[..., 0], f_v, flags, float(margin.min()) if margin.size else float("inf")), \
        (om_e, lam_e, None if c_e is None else c_e[..., 0], f_e)


def switching_information_step(model, regime_next, info, y, dtype=np.float64):
    """(Om [B,N,D(D+1)/2], lam [B,N,D], c [B,N], F [B,N,D(D+1)/2], flags, margin) of one information step
    (include/aesmc_hip.h: aesmc_switching_information_step, K34) — the comment above states the arithmetic.

    model: `operands`' dict (the probabilities are not read); regime_next: int32 [B,N], the trajectories' regimes s'_{t+1};
    info: None (the last step's zeros) or (Om, lam, c) of time t+1; y: [B,Dy], the observation of time t+1, float32 or
    float64, widened.  F is the packed LOWER factor of Om (element (i,k), i >= k, at `tri(i,k)`): Phi = F^T is the upper
    triangle with Phi^T Phi = Om.  A pivot at or below 2^-40 max_i Om_ii gives a zero column; `margin` is the smallest
    |pivot - threshold| / max_i Om_ii over all trajectories and columns — only a column whose pivot lies this close to the
    threshold can be kept on one side and dropped on the other.  A regime outside [0, M): NaN outputs for that trajectory
    and FLAG_INDEX_OUT_OF_RANGE."""
    with np.errstate(all="ignore"):
        return _information(model, regime_next, info, y, dtype, False)[0]


def switching_information_step_bound(model, regime_next, info, y):
    """(bound of Om, of lam, of c, of F), float64: `switching_kalman_step_bound`'s running analysis of the information
    step, 2 * 1.01 times the running bound; the inputs enter exactly.  A dropped column of F is zero on both sides (its
    bound is 0): the bound holds for a device that keeps and drops the same columns (`margin`).  Zero where the output is NaN."""
    with np.errstate(all="ignore"):
        _, errors = _information(model, regime_next, info, y, np.float64, True)
    return tuple(np.where(np.isfinite(e), 2 * 1.01 * e, np.inf) for e in errors)


def _scores(log_Pi, regime_next, factor, lam, particles, log_w, dtype, track):
    regime, mean, cov = (np.asarray(part) for part in particles)
    regime_next, factor, lam = np.asarray(regime_next), np.asarray(factor), np.asarray(lam)
    log_Pi = np.asarray(log_Pi, dtype=np.float64)
    (B, K), N = regime.shape, regime_next.shape[1]
    M, D = log_Pi.shape[0], mean.shape[-1]
    zero = np.zeros((B, N, K), dtype=dtype)
    given = lambda array: (np.broadcast_to(np.asarray(array), (B, N, K)).astype(dtype), zero if track else None)
    one = given(1.0)
    over_n = lambda array: array[:, :, None]      # [B,N] -> [B,N,1]
    over_k = lambda array: array[:, None, :]      # [B,K] -> [B,1,K]
    bad = over_k((regime < 0) | (regime >= M)) | over_n((regime_next < 0) | (regime_next >= M))
    flags = FLAG_INDEX_OUT_OF_RANGE if bad.any() else 0
    prior = log_Pi[np.where((regime < 0) | (regime >= M), 0, regime)[:, None, :],
                   np.where((regime_next < 0) | (regime_next >= M), 0, regime_next)[:, :, None]]
    F = lambda i, k: given(over_n(factor[:, :, tri(i, k)]))      # F_ik, i >= k
    lm_ = [given(over_n(lam[:, :, i])) for i in range(D)]
    m = [given(over_k(mean[:, :, i])) for i in range(D)]
    P = [given(over_k(cov[:, :, e])) for e in range(D * (D + 1) // 2)]
    t = [_chain(given(0.0), [(F(l, i), m[l]) for l in range(i, D)]) for i in range(D)]
    mq = _chain(given(0.0), [(t[i], t[i]) for i in range(D)])
    h = [_chain(lm_[l], [(F(l, i), t[i]) for i in range(l + 1)], negate=True) for l in range(D)]
    lm = _chain(given(0.0), [(lm_[l], m[l]) for l in range(D)])
    hph = _chain(given(0.0), [(h[c], _chain(given(0.0), [(P[tri(c, l)], h[l]) for l in range(D)])) for c in range(D)])
    v, Lam = [], {}
    for i in range(D):
        W = [_chain(given(0.0), [(F(c, i), P[tri(c, l)]) for c in range(i, D)]) for l in range(D)]
        v.append(_chain(given(0.0), [(W[l], h[l]) for l in range(D)]))
        for j in range(i + 1):
            Lam[tri(i, j)] = _chain(given(1.0 if i == j else 0.0), [(W[l], F(l, j)) for l in range(j, D)])
    inv, log_det = [], given(0.0)
    for k in range(D):
        pivot = _chain(Lam[tri(k, k)], [(Lam[tri(k, c)], Lam[tri(k, c)]) for c in range(k)], negate=True)
        Lam[tri(k, k)] = _sqrt(pivot)
        inv.append(_reciprocal(Lam[tri(k, k)]))
        log_det = _chain(log_det, [(_log(Lam[tri(k, k)]), one)])
        for i in range(k + 1, D):
            Lam[tri(i, k)] = _times(_chain(Lam[tri(i, k)], [(Lam[tri(i, c)], Lam[tri(k, c)]) for c in range(k)],
                                           negate=True), inv[k])
    x = []
    for i in range(D):
        x.append(_times(_chain(v[i], [(Lam[tri(i, c)], x[c]) for c in range(i)], negate=True), inv[i]))
    xq = _chain(given(0.0), [(x[i], x[i]) for i in range(D)])
    excluded = np.isneginf(prior)
    base = given(np.where(excluded, 0.0, prior))
    if log_w is not None:
        base = _chain(given(over_k(np.asarray(log_w))), [(base, one)])
    score = _chain(_chain(_chain(_chain(base, [(lm, one)]), [(given(-0.5), mq)]),
                          [(given(0.5), _chain(hph, [(xq, one)], negate=True))]), [(log_det, one)], negate=True)
    value = np.where(bad, np.nan, np.where(excluded, -np.inf, score[0]))
    error = None
    if track:
        error = np.where(bad | excluded, 0.0, score[1]).astype(np.float64)
    return (value, flags), error


def switching_backward_scores(log_Pi, regime_next, factor, lam, particles, log_w=None, dtype=np.float64):
    """(scores [B,N,K], flags) of one backward step (include/aesmc_hip.h: aesmc_switching_backward_scores, K35) — the
    comment above states the arithmetic.

    log_Pi: float64 [M,M], -inf where a probability is 0; regime_next: int32 [B,N]; factor, lam: the information step's F
    [B,N,D(D+1)/2] and lam [B,N,D]; particles: the stored (regime int32 [B,K], mean [B,K,D], cov [B,K,D(D+1)/2]) of step t;
    log_w: [B,K] or None (equal weights: nothing is added).  The trajectory's constant c is left out: it does not change
    the draw.  -inf where log Pi[s, s'] is -inf whatever the rest is; a regime outside [0, M) on either side: NaN and
    FLAG_INDEX_OUT_OF_RANGE."""
    with np.errstate(all="ignore"):
        return _scores(log_Pi, regime_next, factor, lam, particles, log_w, dtype, False)[0]


def switching_backward_scores_bound(log_Pi, regime_next, factor, lam, particles, log_w=None):
    """The bound of `switching_backward_scores` [B,N,K], float64: the running analysis of `switching_kalman_step_bound`, 2 *
    1.01 times the running bound; the inputs enter exactly.  Zero where the score is NaN or -inf by exclusion."""
    with np.errstate(all="ignore"):
        _, error = _scores(log_Pi, regime_next, factor, lam, particles, log_w, np.float64, True)
    return np.where(np.isfinite(error), 2 * 1.01 * error, np.inf)


def categorical_draw(scores, u):
    """(idx int64 [R], margin [R], flags): K21's draw without a transition term, one trajectory per row — scores [R,K],
    u [R]: idx = min(#{k : C_k <= u C_{K-1}}, the last k of positive weight), C the running sum of exp(score - row maximum)
    (zero below -745.2).  A NaN in a row: idx = K and FLAG_NAN_LOG_WEIGHT; no finite maximum: idx = K and
    FLAG_DEGENERATE_ROW.  margin: |u C_{K-1} - C_k| at the nearest step k of the running sum, over C_{K-1} — only a draw
    this close to a step can differ between two evaluations of the scores."""
    scores, u = np.asarray(scores, dtype=np.float64), np.asarray(u, dtype=np.float64)
    R, K = scores.shape
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(scores).any(axis=1)
        top = np.where(nan, 0.0, np.max(np.where(np.isnan(scores), -np.inf, scores), axis=1))
        degenerate = ~nan & ~np.isfinite(top)
        x = scores - np.where(nan | degenerate, 0.0, top)[:, None]
        w = np.where(x > -745.2, np.exp(np.minimum(x, 0.0)), 0.0)
        w = np.where((nan | degenerate)[:, None], 1.0, w)
    running = np.cumsum(w, axis=1)
    position = u * running[:, -1]
    count = (running <= position[:, None]).sum(axis=1)
    last = K - 1 - np.argmax(w[:, ::-1] > 0, axis=1)
    idx = np.where(nan | degenerate, K, np.minimum(count, last)).astype(np.int64)
    margin = np.abs(running - position[:, None]).min(axis=1) / running[:, -1]
    margin = np.where(nan | degenerate, np.inf, margin)
    flags = (FLAG_NAN_LOG_WEIGHT if nan.any() else 0) | (FLAG_DEGENERATE_ROW if degenerate.any() else 0)
    return idx, margin, flags


def switching_backward_pass(filtered, model, observations, uniforms):
    """The whole Rao-Blackwellised backward simulation on replayed uniforms.  filtered: a pass's dict (`switching_pass`: with
    log_weights; `adapted_switching_pass`: without, the stored systems are equally weighted); model: `operands`' dict;
    observations: T x [B,Dy]; uniforms: T x float64 [B,N] (block t draws time t).

    Returns a dict: regimes (T x int32 [B,N]), indices (T x int64 [B,N]: which stored particle), margins (T x [B,N]:
    `categorical_draw`'s, per draw), score_bounds (T x [B,N]: the largest bound of a draw's scores, 0 at T-1 where the
    scores are the stored log-weights), smoothed_regime_probabilities [T,B,M] (the trajectories' frequencies), information
    ((T-1) tuples (Om, lam, c, F), the one of time t at position t), pivot_margins ((T-1) floats) and flags."""
    T = len(observations)
    B, N = np.asarray(uniforms[0]).shape
    M = model["A"].shape[0]
    K = np.asarray(filtered["regimes"][0]).shape[1]
    with np.errstate(divide="ignore"):
        log_Pi = np.log(model["Pi"])
    weights = filtered.get("log_weights")
    out = {"regimes": [None] * T, "indices": [None] * T, "margins": [None] * T, "score_bounds": [None] * T,
           "information": [None] * (T - 1), "pivot_margins": [None] * (T - 1)}
    flags, info, rows = 0, None, np.arange(B)[:, None]
    for t in range(T - 1, -1, -1):
        particles = tuple(np.asarray(filtered[name][t]) for name in ("regimes", "means", "covariances"))
        log_w = None if weights is None else np.asarray(weights[t])
        if t == T - 1:
            scores = np.broadcast_to((np.zeros((B, K)) if log_w is None else log_w)[:, None, :], (B, N, K))
            bound = np.zeros((B, N))
        else:
            om, lam, c, factor, bits, margin = switching_information_step(model, out["regimes"][t + 1], info,
                                                                          observations[t + 1])
            flags |= bits
            info = (om, lam, c)
            out["information"][t], out["pivot_margins"][t] = (om, lam, c, factor), margin
            scores, bits = switching_backward_scores(log_Pi, out["regimes"][t + 1], factor, lam, particles, log_w)
            flags |= bits
            bound = switching_backward_scores_bound(log_Pi, out["regimes"][t + 1], factor, lam, particles, log_w).max(axis=2)
        idx, margin, bits = categorical_draw(scores.reshape(B * N, K), np.asarray(uniforms[t]).reshape(-1))
        flags |= bits
        idx = idx.reshape(B, N)
        out["indices"][t], out["margins"][t], out["score_bounds"][t] = idx, margin.reshape(B, N), bound
        out["regimes"][t] = particles[0][rows, np.minimum(idx, K - 1)].astype(np.int32)
    out["smoothed_regime_probabilities"] = np.stack([
        np.stack([(s == i).mean(axis=1) if N else np.zeros(B) for i in range(M)], axis=1) for s in out["regimes"]])
    out["flags"] = flags
    return out


def _information_sensitivities(model, regime_next, info, y):
    """How an error of (Om, lam) at time t+1 reaches the information step's outputs, to first order (the largest over the
    trajectories), from plain np.linalg on full matrices.  With Oh = Om + C^T R^-1 C, lh = lam + C^T R^-1 (y - d), Q =
    diag(q^2), J = (I + Q Oh)^-1 and g = J^T lh the step is Om' = A^T Oh J A, lam' = A^T (g - Oh J b), so

        dOm'  = (J A)^T dOm (J A)                                    |dOm'|  <= |J A|^2 |dOm|
        dlam' = (J A)^T dlam - (J A)^T dOm (Q g + J b)               |dlam'| <= |J A| |dlam| + |J A| |Q g + J b| |dOm|

    in the spectral norm (the Euclidean norm of a vector).  Returns (oo, ll, lo): the three factors."""
    regime_next = np.asarray(regime_next)
    B, N = regime_next.shape
    M, D = model["A"].shape[0], model["A"].shape[-1]
    j = np.clip(regime_next, 0, M - 1)
    A, C = model["A"][j], model["C"][j]
    q2, r2 = model["q"][j] ** 2, model["r"][j] ** 2
    Om = np.zeros((B, N, D, D)) if info is None else unpack(np.asarray(info[0]), D)
    lam = np.zeros((B, N, D)) if info is None else np.asarray(info[1])
    weighted = np.swapaxes(C, -1, -2) / r2[:, :, None, :]                                  # C^T R^-1
    Oh = Om + weighted @ C
    lh = lam + np.einsum("bnij,bnj->bni", weighted, np.asarray(y, dtype=np.float64)[:, None, :] - model["d"][j])
    J = np.linalg.inv(np.eye(D) + q2[:, :, :, None] * Oh)
    JA = J @ A
    g = np.einsum("bnji,bnj->bni", J, lh)
    carried = q2 * g + np.einsum("bnij,bnj->bni", J, model["b"][j])
    norm = np.linalg.norm(JA, 2, axis=(-2, -1))
    return float((norm * norm).max()), float(norm.max()), float((norm * np.linalg.norm(carried, axis=-1)).max())


def switching_information_pass(model, regimes, observations):
    """The information steps of T-1 .. 1 chained along GIVEN regime paths (no draws): regimes T x int32 [B,N], observations
    T x [B,Dy].  Returns a dict: information ((T-1) tuples (Om, lam, c, F), the one of time t at position t), pivot_margins
    ((T-1) floats), flags, and tolerances {"omega": (T-1) floats, "lambda": (T-1) floats}, propagated as `switching_pass`
    propagates the filter's — how far a device run whose launches stay within their bounds may lie from this one, on the
    spectral norm of a trajectory's Om error and the Euclidean norm of its lam error; with the factors of
    `_information_sensitivities`, the step's own bound in the Frobenius norm, and 1.01 for the terms of second order:

        tol_Om[t]  = 1.01 oo tol_Om[t+1] + max |Om bound|_F
        tol_lam[t] = 1.01 (ll tol_lam[t+1] + lo tol_Om[t+1]) + max |lam bound|_2."""
    T = len(observations)
    D = model["A"].shape[-1]
    out = {"information": [None] * (T - 1), "pivot_margins": [None] * (T - 1), "flags": 0,
           "tolerances": {"omega": [None] * (T - 1), "lambda": [None] * (T - 1)}}
    info, tol_o, tol_l = None, 0.0, 0.0
    for t in range(T - 2, -1, -1):
        om, lam, c, factor, bits, margin = switching_information_step(model, regimes[t + 1], info, observations[t + 1])
        bound_o, bound_l, _, _ = switching_information_step_bound(model, regimes[t + 1], info, observations[t + 1])
        fresh_o = float(np.sqrt((unpack(bound_o, D) ** 2).sum(axis=(-2, -1))).max())
        fresh_l = float(np.sqrt((bound_l ** 2).sum(axis=-1)).max())
        if info is None:
            tol_o, tol_l = fresh_o, fresh_l
        else:
            oo, ll, lo = _information_sensitivities(model, regimes[t + 1], info, observations[t + 1])
            tol_o, tol_l = 1.01 * oo * tol_o + fresh_o, 1.01 * (ll * tol_l + lo * tol_o) + fresh_l
        info = (om, lam, c)
        out["information"][t], out["pivot_margins"][t] = (om, lam, c, factor), margin
        out["tolerances"]["omega"][t], out["tolerances"]["lambda"][t] = tol_o, tol_l
        out["flags"] |= bits
    return out


def exact_regime_marginals(model, ys):
    """p(s_t = i | y_0..y_{T-1}) [T,M] of ONE series (ys: T x [Dy]) by enumerating all M^T regime sequences, each an exact
    Kalman filter — `exact_log_likelihood`'s terms, normalised and summed per (t, regime)."""
    ys = [np.asarray(y, dtype=np.float64).reshape(1, -1) for y in ys]
    T, M = len(ys), model["A"].shape[0]
    sequences = list(itertools.product(range(M), repeat=T))
    terms = np.empty(len(sequences))
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    for position, sequence in enumerate(sequences):
        prior = log_pi0[sequence[0]] + sum(log_Pi[a, b] for a, b in zip(sequence, sequence[1:]))
        terms[position] = prior + _sequence_log_likelihood(model, sequence, ys)
    weights = np.exp(terms - terms.max())
    weights /= weights.sum()
    marginals = np.zeros((T, M))
    for weight, sequence in zip(weights, sequences):
        for t, s in enumerate(sequence):
            marginals[t, s] += weight
    return marginals


def _sequence_log_likelihood(model, sequence, ys):
    """log p(y_0..y_{T-1} | s_0..s_{T-1}) of one series by the Kalman filter (plain np.linalg on full matrices)."""
    D, Dy = model["A"].shape[-1], model["C"].shape[-2]
    mean, cov, total = model["m0"].copy(), np.diag(model["s0"] ** 2), 0.0
    for t, s in enumerate(sequence):
        A, C = model["A"][s], model["C"][s]
        if t > 0:
            mean, cov = A @ mean + model["b"][s], A @ cov @ A.T + np.diag(model["q"][s] ** 2)
        S = C @ cov @ C.T + np.diag(model["r"][s] ** 2)
        residual = ys[t][0] - C @ mean - model["d"][s]
        total -= 0.5 * (residual @ np.linalg.solve(S, residual) + np.linalg.slogdet(S)[1] + 2 * Dy * HALF_LOG_2PI)
        gain = cov @ C.T @ np.linalg.inv(S)
        mean, cov = mean + gain @ residual, cov - gain @ C @ cov
    return total


# (B, K, N, M, D, Dy): `STEP_SHAPES` with a number of trajectories each — one lane; a partial tile of trajectories; a tile of
# particles that is not full beside every padded extent; more than one tile of trajectories; the largest M; several tiles
# of particles
BACKWARD_SHAPES = [(1, 1, 1, 1, 1, 1), (3, 7, 5, 2, 2, 1), (2, 65, 9, 3, 8, 8), (2, 300, 17, 4, 5, 3), (1, 257, 8, 16, 8, 1),
                   (2, 1025, 3, 2, 3, 2)]


def example_backward_step(B, K, N, M, D, Dy, steps=1, observation_dtype=np.float64, seed=0):
    """(model, regime_next, info, y, particles, log_w) of one backward step: `example_step`'s model and stored particles,
    random regimes for the trajectories, and `info` the result of `steps - 1` information steps from the zeros of the last
    timestep (steps = 1: None, the first step; with Dy < D the Om that steps = 2 hands over is rank-deficient)."""
    model, particles, _, _, _ = example_step(B, K, M, D, Dy, seed=seed)
    rng = np.random.default_rng([seed, B, K, N, M, D, Dy, 34])
    info = None
    for _ in range(steps - 1):
        om, lam, c, _, _, _ = switching_information_step(model, rng.integers(0, M, (B, N)).astype(np.int32), info,
                                                         rng.standard_normal((B, Dy)))
        info = (om, lam, c)
    regime_next = rng.integers(0, M, (B, N)).astype(np.int32)
    y = rng.standard_normal((B, Dy)).astype(observation_dtype)
    return model, regime_next, info, y, particles, rng.standard_normal((B, K))


# ---- the smoothed continuous state: the two-filter combination (K36) and the pass it makes with K31 and K34 ------------------------
# Given a regime trajectory the model is linear-Gaussian and its state smoother exact (Fong, Godsill, Doucet & West 2002;
# Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016).  At time t the trajectory has the conditional Kalman filter's N(m, P) (the
# step under `_forced`) and the information step's (F, lam) of time t, Om = F F^T.  Their product is N(m^s, P^s), per trajectory
# (sums and packing as above):
#
#     t_i  = sum_{l>=i} F_li m_l;   h_l = lam_l - sum_{i<=l} F_li t_i
#     W_il = sum_{c>=i} F_ci P_cl;  Lam_ij = (i == j) + sum_{l>=j} W_il F_lj   (j <= i; pivots at least 1)
#     G = chol(Lam);  U_il = (W_il - sum_{c<i} G_ic U_cl) / G_ii
#     P^s_pq = P_pq - sum_i U_ip U_iq;   m^s_p = m_p + sum_l P^s_pl h_l
#
# and, with j = s'_{t+1}, the smoothed P^s_{t+1} and the information step's Om_{t+1} (zeros at t+1 = T-1), the lag-one
# cross-covariance Cov(z_{t+1,i}, z_{t,l} | y, s) — the off-diagonal block of (Sigma^-1 + diag(0, Oh))^-1 for the joint Sigma of
# (z_t, z_{t+1}) given y_{0:t}, which inverts no predicted covariance (q = 0 and P = 0 are fine):
#
#     rho_i = 1 / r_j[i]^2;  Gc_il = C_j[i,l] rho_i;  Oh_pq = Om_{t+1,pq} + sum_i Gc_ip C_j[i,q]
#     V_il = sum_c A_j[i,c] P_cl;   Y_pl = sum_q Oh_pq V_ql;   cross_il = V_il - sum_p P^s_{t+1,ip} Y_pl
def _combine(model, regime_next, filtered, factor, lam, omega_next, cov_next, dtype, track):
    mean_in, cov_in = (np.asarray(part) for part in filtered)
    factor, lam = np.asarray(factor), np.asarray(lam)
    B, N, D = mean_in.shape
    TD = D * (D + 1) // 2
    zero = np.zeros((B, N), dtype=dtype)
    given = lambda array: (np.asarray(array).astype(dtype), zero if track else None)
    m = [given(mean_in[:, :, i]) for i in range(D)]
    P = [given(cov_in[:, :, e]) for e in range(TD)]
    Fv = [given(factor[:, :, e]) for e in range(TD)]
    F = lambda i, k: Fv[tri(i, k)]      # F_ik, i >= k
    lm = [given(lam[:, :, i]) for i in range(D)]
    t = [_chain(given(zero), [(F(l, i), m[l]) for l in range(i, D)]) for i in range(D)]
    h = [_chain(lm[l], [(F(l, i), t[i]) for i in range(l + 1)], negate=True) for l in range(D)]
    W = [[_chain(given(zero), [(F(c, i), P[tri(c, l)]) for c in range(i, D)]) for l in range(D)] for i in range(D)]
    Lam = {}
    for i in range(D):
        for j in range(i + 1):
            Lam[tri(i, j)] = _chain(given(zero + (1.0 if i == j else 0.0)), [(W[i][l], F(l, j)) for l in range(j, D)])
    inv = []
    for k in range(D):
        pivot = _chain(Lam[tri(k, k)], [(Lam[tri(k, c)], Lam[tri(k, c)]) for c in range(k)], negate=True)
        Lam[tri(k, k)] = _sqrt(pivot)
        inv.append(_reciprocal(Lam[tri(k, k)]))
        for i in range(k + 1, D):
            Lam[tri(i, k)] = _times(_chain(Lam[tri(i, k)], [(Lam[tri(i, c)], Lam[tri(k, c)]) for c in range(k)],
                                           negate=True), inv[k])
    U = []
    for i in range(D):
        U.append([_times(_chain(W[i][l], [(Lam[tri(i, c)], U[c][l]) for c in range(i)], negate=True), inv[i])
                  for l in range(D)])
    S = [_chain(P[tri(p, q)], [(U[i][p], U[i][q]) for i in range(D)], negate=True) for p in range(D) for q in range(p + 1)]
    ms = [_chain(m[p], [(S[tri(p, l)], h[l]) for l in range(D)]) for p in range(D)]
    bad, flags, X = np.zeros((B, N), dtype=bool), 0, None
    if cov_next is not None:
        regime_next = np.asarray(regime_next)
        M, Dy = model["A"].shape[0], model["C"].shape[-2]
        bad = (regime_next < 0) | (regime_next >= M)
        flags = FLAG_INDEX_OUT_OF_RANGE if bad.any() else 0
        j = np.where(bad, 0, regime_next)
        A, C, r = (model[name][j] for name in ("A", "C", "r"))
        Am = [[given(A[:, :, i, l]) for l in range(D)] for i in range(D)]
        Cm = [[given(C[:, :, i, l]) for l in range(D)] for i in range(Dy)]
        rho = [_reciprocal(given(r[:, :, i] * r[:, :, i])) for i in range(Dy)]
        Gc = [[_times(Cm[i][l], rho[i]) for l in range(D)] for i in range(Dy)]
        Om = [given(zero)] * TD if omega_next is None else [given(np.asarray(omega_next)[:, :, e]) for e in range(TD)]
        Oh = [_chain(Om[tri(a, b)], [(Gc[i][a], Cm[i][b]) for i in range(Dy)]) for a in range(D) for b in range(a + 1)]
        Sn = [given(np.asarray(cov_next)[:, :, e]) for e in range(TD)]
        V = [[_chain(given(zero), [(Am[i][c], P[tri(c, l)]) for c in range(D)]) for l in range(D)] for i in range(D)]
        Y = [[_chain(given(zero), [(Oh[tri(p, q)], V[q][l]) for q in range(D)]) for l in range(D)] for p in range(D)]
        X = [_chain(V[i][l], [(Sn[tri(i, p)], Y[p][l]) for p in range(D)], negate=True) for i in range(D) for l in range(D)]

    def finish(parts):
        values = np.stack([part[0] for part in parts], axis=-1)
        values[bad] = np.nan
        errors = None
        if track:
            errors = np.stack([part[1] for part in parts], axis=-1).astype(np.float64)
            errors[bad] = 0.0
        return values, errors

    (mean_v, mean_e), (cov_v, cov_e) = finish(ms), finish(S)
    cross_v = cross_e = None
    if X is not None:
        cross_v, cross_e = finish(X)
        cross_v = cross_v.reshape(B, N, D, D)
        cross_e = None if cross_e is None else cross_e.reshape(B, N, D, D)
    return (mean_v, cov_v, cross_v, flags), (mean_e, cov_e, cross_e)


def switching_smooth_combine(model, regime_next, filtered, factor, lam, omega_next, cov_next, dtype=np.float64):
    """(mean [B,N,D], cov [B,N,D(D+1)/2], cross [B,N,D,D] or None, flags) of one combination (include/aesmc_hip.h:
    aesmc_switching_smooth_combine, K36) — the comment above states the arithmetic.

    filtered: (mean [B,N,D], cov [B,N,D(D+1)/2]), the conditional filter's of time t; factor, lam: the information step's F
    and lam of time t.  The cross-covariance is formed when `cov_next` (the smoothed packed covariance of time t+1) is given:
    model: `operands`' dict (A, C, r are read); regime_next int32 [B,N]; omega_next: the information step's Om of time t+1 or
    None (t+1 = T-1: zeros).  With cov_next None the cross-covariance is None and model, regime_next and omega_next are not
    read (pass None).  cross[b,n,i,l] = Cov(z_{t+1,i}, z_{t,l}).  A regime outside [0, M), where it is read: NaN in all three
    outputs of that trajectory and FLAG_INDEX_OUT_OF_RANGE."""
    with np.errstate(all="ignore"):
        return _combine(model, regime_next, filtered, factor, lam, omega_next, cov_next, dtype, False)[0]


def switching_smooth_combine_bound(model, regime_next, filtered, factor, lam, omega_next, cov_next):
    """(bound of mean, of cov, of cross or None), float64: `switching_kalman_step_bound`'s running analysis of the
    combination, 2 * 1.01 times the running bound; the inputs enter exactly.  Zero where the output is NaN."""
    with np.errstate(all="ignore"):
        _, errors = _combine(model, regime_next, filtered, factor, lam, omega_next, cov_next, np.float64, True)
    return tuple(None if e is None else np.where(np.isfinite(e), 2 * 1.01 * e, np.inf) for e in errors)


def _combine_sensitivities(model, regime_next, filtered, factor, lam, omega_next, cov_next):
    """How errors of its inputs reach the combination's outputs, to first order (the largest over the trajectories), from
    plain np.linalg on full matrices.  With Om = F F^T, J = (I + P Om)^-1, P^s = J P, m^s = J (m + P lam), h = lam - Om m:

        dP^s = J dP J^T - P^s dOm P^s                          |dP^s| <= |J|^2 |dP| + |P^s|^2 |dOm|
        dm^s = J dm + P^s dlam - P^s dOm m^s + J dP J^T h      |dm^s| <= |J| |dm| + |P^s| |dlam| + |P^s| |m^s| |dOm| + |J| |J^T h| |dP|

    and with Oh = Om_{t+1} + C^T R^-1 C, cross = (I - P^s_{t+1} Oh) A P:

        dcross = (I - P^s_{t+1} Oh) A dP - dP^s_{t+1} Oh A P - P^s_{t+1} dOm_{t+1} A P
        |dcross| <= |(I - P^s_{t+1} Oh) A| |dP| + |Oh A P| |dP^s_{t+1}| + |P^s_{t+1}| |A P| |dOm_{t+1}|

    in the spectral norm (the Euclidean norm of a vector).  Returns (pp, po, mm, ml, mo, mp) and (xp, xs, xo) — the second
    triple None without cov_next."""
    mean, cov = filtered
    B, N, D = mean.shape
    P = unpack(np.asarray(cov), D)
    lower = np.tril(unpack(np.asarray(factor), D))
    Om = lower @ np.swapaxes(lower, -1, -2)
    J = np.linalg.inv(np.eye(D) + P @ Om)
    Ps = J @ P
    h = lam - np.einsum("bnij,bnj->bni", Om, mean)
    ms = mean + np.einsum("bnij,bnj->bni", Ps, h)
    norm = lambda matrix: np.linalg.norm(matrix, 2, axis=(-2, -1))
    nj, ns = norm(J), norm(Ps)
    first = (float((nj * nj).max()), float((ns * ns).max()), float(nj.max()), float(ns.max()),
             float((ns * np.linalg.norm(ms, axis=-1)).max()),
             float((nj * np.linalg.norm(np.einsum("bnji,bnj->bni", J, h), axis=-1)).max()))
    if cov_next is None:
        return first, None
    M = model["A"].shape[0]
    j = np.clip(regime_next, 0, M - 1)
    A, C, r2 = model["A"][j], model["C"][j], model["r"][j] ** 2
    Oh = (np.zeros((B, N, D, D)) if omega_next is None else unpack(np.asarray(omega_next), D)) + \
        (np.swapaxes(C, -1, -2) / r2[:, :, None, :]) @ C
    Sn = unpack(np.asarray(cov_next), D)
    V = A @ P
    return first, (float(norm((np.eye(D) - Sn @ Oh) @ A).max()), float(norm(Oh @ V).max()), float((norm(Sn) * norm(V)).max()))


def _dropped_amplification(omega, factor, D):
    """(1 + |Om_KK^+ Om_KZ|)^2, the largest over the trajectories: how an error of Om reaches what the factor DROPS (the Schur
    complement of the kept columns K in the dropped ones Z), to first order; 1 where nothing is dropped."""
    full, lower = unpack(np.asarray(omega), D), np.tril(unpack(np.asarray(factor), D))
    worst = 1.0
    kept = lower[..., np.arange(D), np.arange(D)] > 0
    for index in np.argwhere(~kept.all(axis=-1)):
        keep = kept[tuple(index)]
        if keep.any():
            block = full[tuple(index)]
            solved = np.linalg.lstsq(block[np.ix_(keep, keep)], block[np.ix_(keep, ~keep)], rcond=None)[0]
            worst = max(worst, (1.0 + float(np.linalg.norm(solved, 2))) ** 2)
    return worst


def switching_state_pass(model, regimes, observations):
    """The state smoother along GIVEN regime paths (no draws): the conditional Kalman filter forward (`switching_kalman_step`
    under `_forced`, one particle per trajectory, no ancestors), `switching_information_pass` backward, and the combination
    at every t < T-1 (at T-1 the smoothed moments are the filtered ones).  regimes: T x int32 [B,N]; observations: T x [B,Dy].

    Returns a dict: means (T x [B,N,D]), covariances (T x [B,N,D(D+1)/2]), cross_covariances ((T-1) x [B,N,D,D], the one of
    (t+1, t) at position t), log_likelihood [B,N] (log p(y | s_{0:T-1}): the steps' log-weights summed in time order),
    filtered_means, filtered_covariances (T each), information (`switching_information_pass`'s), pivot_margins, flags, and
    tolerances, propagated as `switching_pass` and `switching_information_pass` propagate theirs — how far a device run
    whose launches stay within their bounds may lie from this one: `filtered_means`, `filtered_covariances` (T floats each,
    `switching_pass`'s recurrences), `log_likelihood` (one float: the steps' summed, plus T u |log_likelihood| for the sums),
    `means`, `covariances` (T floats each) and `cross_covariances` (T-1 floats): on the Euclidean norm of a trajectory's mean
    error and the spectral norm of its (cross-)covariance error, which bound every element's.  With the factors of
    `_combine_sensitivities`, the combination's own bound in the Frobenius norm, 1.01 for the terms of second order, tol_m,
    tol_P the filter's and tol_lam, tol_Om the information pass's:

        tol_FF[t]  = 1.01 amp tol_Om[t] + max 2 |F|_F |F bound|_F       (of F F^T, which the combination reads in place of Om:
                                                                         `_dropped_amplification` for what the factor drops)
        tol_Ps[t]  = 1.01 (pp tol_P[t] + po tol_FF[t]) + max |cov bound|_F
        tol_ms[t]  = 1.01 (mm tol_m[t] + ml tol_lam[t] + mo tol_FF[t] + mp tol_P[t]) + max |mean bound|_2
        tol_x[t]   = 1.01 (xp tol_P[t] + xs tol_Ps[t+1] + xo tol_Om[t+1]) + max |cross bound|_F      (tol_Om[T-1] = 0)."""
    T = len(observations)
    regimes = [np.asarray(regime).astype(np.int32) for regime in regimes]
    D = model["A"].shape[-1]
    frob = lambda packed: float(np.sqrt((unpack(packed, D) ** 2).sum(axis=(-2, -1))).max())
    two = lambda vector: float(np.sqrt((vector ** 2).sum(axis=-1)).max())
    filtered_m, filtered_p, tol_m, tol_p = [], [], [], []
    state, flags, total, tol_total = None, 0, 0.0, 0.0
    for t in range(T):
        shim, forced = _forced(model, regimes[t])
        regime, mean, cov, log_w, bits = switching_kalman_step(shim, state, None, forced, observations[t])
        bound_m, bound_p, bound_w = switching_kalman_step_bound(shim, state, None, forced, observations[t])
        flags |= bits
        if t == 0:
            tm, tp, tw = two(bound_m), frob(bound_p), float(bound_w.max())
        else:
            pp, mm, mp, wm, wp = _sensitivities(shim, state, None, regime, observations[t])
            tm = 1.01 * (mm * tol_m[-1] + mp * tol_p[-1]) + two(bound_m)
            tw = 1.01 * (wm * tol_m[-1] + wp * tol_p[-1]) + float(bound_w.max())
            tp = 1.01 * pp * tol_p[-1] + frob(bound_p)
        state = (regime, mean, cov)
        total = total + log_w
        tol_total += tw
        filtered_m.append(mean), filtered_p.append(cov), tol_m.append(tm), tol_p.append(tp)
    with np.errstate(invalid="ignore"):
        tol_total += T * UNIT * float(np.nanmax(np.abs(total))) if np.isfinite(total).any() else 0.0
    backward = switching_information_pass(model, regimes, observations)
    flags |= backward["flags"]
    means, covs, crosses = [None] * T, [None] * T, [None] * (T - 1)
    tol_ms, tol_ps, tol_x = [None] * T, [None] * T, [None] * (T - 1)
    means[T - 1], covs[T - 1], tol_ms[T - 1], tol_ps[T - 1] = filtered_m[-1], filtered_p[-1], tol_m[-1], tol_p[-1]
    for t in range(T - 2, -1, -1):
        om, lam, _, factor = backward["information"][t]
        later = t + 1 < T - 1
        omega_next = backward["information"][t + 1][0] if later else None
        args = (model, regimes[t + 1], (filtered_m[t], filtered_p[t]), factor, lam, omega_next, covs[t + 1])
        means[t], covs[t], crosses[t], bits = switching_smooth_combine(*args)
        bound_m, bound_p, bound_x = switching_smooth_combine_bound(*args)
        flags |= bits
        with np.errstate(invalid="ignore"):
            (pp, po, mm, ml, mo, mp), (xp, xs, xo) = _combine_sensitivities(*args)
        _, _, _, bound_f = switching_information_step_bound(model, regimes[t + 1], None if not later else
                                                            backward["information"][t + 1][:3], observations[t + 1])
        tol_om, tol_lam = backward["tolerances"]["omega"][t], backward["tolerances"]["lambda"][t]
        tol_ff = 1.01 * _dropped_amplification(om, factor, D) * tol_om + \
            float((2.0 * np.sqrt((np.tril(unpack(factor, D)) ** 2).sum(axis=(-2, -1))) *
                   np.sqrt((np.tril(unpack(bound_f, D)) ** 2).sum(axis=(-2, -1)))).max())
        tol_ps[t] = 1.01 * (pp * tol_p[t] + po * tol_ff) + frob(bound_p)
        tol_ms[t] = 1.01 * (mm * tol_m[t] + ml * tol_lam + mo * tol_ff + mp * tol_p[t]) + two(bound_m)
        tol_x[t] = 1.01 * (xp * tol_p[t] + xs * tol_ps[t + 1] +
                           xo * (backward["tolerances"]["omega"][t + 1] if later else 0.0)) + \
            float(np.sqrt((bound_x ** 2).sum(axis=(-2, -1))).max())
    return {"means": means, "covariances": covs, "cross_covariances": crosses, "log_likelihood": total,
            "filtered_means": filtered_m, "filtered_covariances": filtered_p, "information": backward["information"],
            "pivot_margins": backward["pivot_margins"], "flags": flags,
            "tolerances": {"filtered_means": tol_m, "filtered_covariances": tol_p, "log_likelihood": float(tol_total),
                           "means": tol_ms, "covariances": tol_ps, "cross_covariances": tol_x}}


def exact_state_smoother(model, sequence, ys):
    """(means [T,D], covariances [T,D,D], cross_covariances [T-1,D,D]) of ONE series (ys: T x [Dy]) under ONE regime sequence:
    the dense joint Gaussian of (z_0..z_{T-1}, y_0..y_{T-1}) conditioned on the observations with plain np.linalg — the
    independent statement of what the pass computes.  cross_covariances[t][i,l] = Cov(z_{t+1,i}, z_{t,l} | y)."""
    T = len(sequence)
    D, Dy = model["A"].shape[-1], model["C"].shape[-2]
    mu, Sigma = np.zeros(T * D), np.zeros((T * D, T * D))
    at = lambda t: slice(t * D, (t + 1) * D)
    for t, s in enumerate(sequence):
        if t == 0:
            mu[at(0)], Sigma[at(0), at(0)] = model["m0"], np.diag(model["s0"] ** 2)
            continue
        A = model["A"][s]
        mu[at(t)] = A @ mu[at(t - 1)] + model["b"][s]
        Sigma[at(t), :t * D] = A @ Sigma[at(t - 1), :t * D]
        Sigma[:t * D, at(t)] = Sigma[at(t), :t * D].T
        Sigma[at(t), at(t)] = A @ Sigma[at(t - 1), at(t - 1)] @ A.T + np.diag(model["q"][s] ** 2)
    H, offset, R = np.zeros((T * Dy, T * D)), np.zeros(T * Dy), np.zeros(T * Dy)
    for t, s in enumerate(sequence):
        rows = slice(t * Dy, (t + 1) * Dy)
        H[rows, at(t)], offset[rows], R[rows] = model["C"][s], model["d"][s], model["r"][s] ** 2
    y = np.concatenate([np.asarray(part, dtype=np.float64).reshape(-1) for part in ys])
    Szy = Sigma @ H.T
    Syy = H @ Szy + np.diag(R)
    mean = mu + Szy @ np.linalg.solve(Syy, y - H @ mu - offset)
    cov = Sigma - Szy @ np.linalg.solve(Syy, Szy.T)
    return (np.stack([mean[at(t)] for t in range(T)]), np.stack([cov[at(t), at(t)] for t in range(T)]),
            np.stack([cov[at(t + 1), at(t)] for t in range(T - 1)]) if T > 1 else np.zeros((0, D, D)))


def exact_smoothed_state(model, ys):
    """(E[z_t | y] [T,D], Cov[z_t | y] [T,D,D], E[z_{t+1} z_t^T | y] [T-1,D,D]) of ONE series (ys: T x [Dy]): the mixture of
    `exact_state_smoother` over all M^T regime sequences with `exact_regime_marginals`' weights (the sequences' posterior
    probabilities)."""
    rows = [np.asarray(y, dtype=np.float64).reshape(1, -1) for y in ys]
    T, M, D = len(rows), model["A"].shape[0], model["A"].shape[-1]
    sequences = list(itertools.product(range(M), repeat=T))
    terms = np.empty(len(sequences))
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    for position, sequence in enumerate(sequences):
        prior = log_pi0[sequence[0]] + sum(log_Pi[a, b] for a, b in zip(sequence, sequence[1:]))
        terms[position] = prior + _sequence_log_likelihood(model, sequence, rows)
    weights = np.exp(terms - terms.max())
    weights /= weights.sum()
    first, second, lagged = np.zeros((T, D)), np.zeros((T, D, D)), np.zeros((max(T - 1, 0), D, D))
    for weight, sequence in zip(weights, sequences):
        if weight == 0.0:
            continue
        mean, cov, cross = exact_state_smoother(model, sequence, ys)
        first += weight * mean
        second += weight * (cov + mean[:, :, None] * mean[:, None, :])
        if T > 1:
            lagged += weight * (cross + mean[1:, :, None] * mean[:-1, None, :])
    return first, second - first[:, :, None] * first[:, None, :], lagged


def example_smooth_combine(B, N, M, D, Dy, steps=1, seed=0):
    """(model, regime_next, filtered, factor, lam, omega_next, cov_next) of one combination at a time t: `example_model`, the
    information of time t after `steps` information steps from the zeros of the last timestep (steps = 1: t+1 = T-1 and
    omega_next None; steps = 2: with Dy < D the Om of time t+1 is rank-deficient), a standard-normal filtered mean and
    filtered and next smoothed covariances F F^T / D + 0.1 I."""
    model, regime_next, info, y, _, _ = example_backward_step(B, 1, N, M, D, Dy, steps=steps, seed=seed)
    _, lam, _, factor, _, _ = switching_information_step(model, regime_next, info, y)
    rng = np.random.default_rng([seed, B, N, M, D, Dy, 36])

    def covariance():
        root = rng.standard_normal((B, N, D, D))
        return np.ascontiguousarray(pack(root @ np.swapaxes(root, -1, -2) / D + 0.1 * np.eye(D)))

    filtered = (rng.standard_normal((B, N, D)), covariance())
    return model, regime_next, filtered, factor, lam, None if info is None else info[0], covariance()


# ---- particle Gibbs on the regimes: conditional resampling (K37), the conditional step (K38) and the sweep they make -------------
# Conditional SMC (Andrieu, Doucet & Holenstein 2010) on the regimes of the Rao-Blackwellised filter: slot K-1 carries a
# reference regime path s'_0..s'_{T-1}.  With z integrated out the regimes are not Markov, so the ancestor-sampling weight of
# stored particle j at the step entering time t is (Whiteley, Andrieu & Doucet 2010; Lindsten, Bunch, Saerkkae, Schoen &
# Godsill 2016)
#
#     w_j Pi[s_j, s'_t] p(y_{t..T-1} | s'_{t..T-1}, m_j, P_j)
#
# — exactly `switching_backward_scores` of the ONE trajectory s' against the information (F, lam) that
# `switching_information_step` carries backwards along it, with log w included.
def _step_margins(w, bad, u):
    """|u C[K-1] - C[j]| at the nearest step j of the running sum, over C[K-1], per row and column of u [B,R]; inf for a bad
    row.  Only a draw this close to a step can differ between two evaluations of the weights."""
    B, K = w.shape
    running = np.cumsum(np.where(bad[:, None], 1.0, w), axis=1)
    out = np.full(u.shape, np.inf)
    for b in range(B):
        if bad[b] or u.shape[1] == 0:
            continue
        position = u[b] * running[b, -1]
        right = np.minimum(np.searchsorted(running[b], position, side="left"), K - 1)
        left = np.maximum(right - 1, 0)
        out[b] = np.minimum(np.abs(running[b, right] - position), np.abs(running[b, left] - position)) / running[b, -1]
    return out


def switching_conditional_ancestor_index(log_w, u, log_Pi, regime_next, factor, lam, particles):
    """(idx int64 [B,K], flags, margins [B,K], score_bound [B]) of one conditional resampling step (include/aesmc_hip.h:
    aesmc_switching_conditional_ancestor_index, K37).

    log_w, u: float64 [B,K]; log_Pi: float64 [M,M]; regime_next: int32 [B], the reference's regime at the step being
    entered; factor [B,D(D+1)/2], lam [B,D]: `switching_information_step`'s F and lam of the reference (N = 1, squeezed), or
    both None (no ancestor sampling); particles: the stored (regime, mean, cov) the weights belong to.

        idx[b,k]   = `testing.particle_gibbs.conditional_ancestor_index`'s free slots, k = 0 .. K-2
        idx[b,K-1] = K - 1 without ancestor sampling; else the same draw at u[b,K-1] over
                     s[j] = switching_backward_scores(log_Pi, regime_next[:,None], factor[:,None], lam[:,None], particles,
                                                      log_w)[b,0,j]

    Bad rows as that function's: a NaN among log_w — FLAG_NAN_LOG_WEIGHT, every slot K; no finite maximum —
    FLAG_DEGENERATE_ROW, every slot K; the same among s, where only idx[b,K-1] = K.  A regime outside [0, M) on either side:
    NaN scores and FLAG_INDEX_OUT_OF_RANGE beside them.
    margins: `_step_margins` of every draw (inf where nothing is drawn); score_bound: the largest
    `switching_backward_scores_bound` among a row's finite scores (0 without ancestor sampling)."""
    from . import particle_gibbs as _pg
    log_w = np.asarray(log_w, dtype=np.float64)
    B, K = log_w.shape
    u = np.asarray(u, dtype=np.float64)
    if u.shape != (B, K):
        raise ValueError("one uniform per slot: u must be [{}, {}], got {}".format(B, K, u.shape))
    if (factor is None) != (lam is None):
        raise ValueError("factor and lam come together")
    w, nan, degenerate = _pg._weights(log_w)
    flags = (FLAG_NAN_LOG_WEIGHT if nan.any() else 0) | (FLAG_DEGENERATE_ROW if degenerate.any() else 0)
    bad_row = nan | degenerate
    idx = np.empty((B, K), dtype=np.int64)
    margins = np.full((B, K), np.inf)
    idx[:, :K - 1] = _pg._draw(w, bad_row, u[:, :K - 1])
    margins[:, :K - 1] = _step_margins(w, bad_row, u[:, :K - 1])
    if factor is None:
        idx[:, K - 1] = np.where(bad_row, K, K - 1)
        return idx, flags, margins, np.zeros(B)
    args = (log_Pi, np.asarray(regime_next).reshape(B, 1), np.asarray(factor)[:, None, :], np.asarray(lam)[:, None, :],
            particles, log_w)
    scores, bits = switching_backward_scores(*args)
    scores = scores[:, 0, :]
    bound = np.where(np.isfinite(scores), switching_backward_scores_bound(*args)[:, 0, :], 0.0).max(axis=1)
    flags |= bits
    w, nan, degenerate = _pg._weights(scores)
    flags |= (FLAG_NAN_LOG_WEIGHT if nan.any() else 0) | (FLAG_DEGENERATE_ROW if degenerate.any() else 0)
    pinned = _pg._draw(w, nan | degenerate, u[:, K - 1:])[:, 0]
    idx[:, K - 1] = np.where(bad_row, K, pinned)
    margins[:, K - 1] = np.where(bad_row, np.inf, _step_margins(w, nan | degenerate, u[:, K - 1:])[:, 0])
    return idx, flags, margins, bound


def _conditional_step(model, state, idx, uniforms, pinned_regime, y, dtype, track):
    """`_step`, and `_step` under `_forced` for the pinned regime, whose slot K-1 replaces the first's."""
    uniforms = np.asarray(uniforms, dtype=np.float64)
    B, K = uniforms.shape
    M = model["A"].shape[0]
    pinned_regime = np.asarray(pinned_regime)
    outside = (pinned_regime < 0) | (pinned_regime >= M)
    shim, forced = _forced(model, np.broadcast_to(np.where(outside, 0, pinned_regime)[:, None], (B, K)))
    (regime, mean, cov, log_w, flags), errors = _step(model, state, idx, uniforms, y, dtype, track)
    (regime_p, mean_p, cov_p, log_w_p, _), errors_p = _step(shim, state, idx, forced, y, dtype, track)
    regime, mean, cov, log_w = regime.copy(), mean.copy(), cov.copy(), log_w.copy()
    regime[:, K - 1], mean[:, K - 1], cov[:, K - 1], log_w[:, K - 1] = regime_p[:, K - 1], mean_p[:, K - 1], cov_p[:, K - 1], \
        log_w_p[:, K - 1]
    regime[outside, K - 1], mean[outside, K - 1], cov[outside, K - 1], log_w[outside, K - 1] = 0, np.nan, np.nan, np.nan
    if track:
        for e, e_p in zip(errors, errors_p):
            e[:, K - 1] = e_p[:, K - 1]
            e[outside, K - 1] = 0.0
    # the flag of slot K-1 is its own: its ancestor, its stored regime, its pinned regime
    if state is None:
        bad = np.zeros((B, K), dtype=bool)
    else:
        ancestors = np.broadcast_to(np.arange(K), (B, K)) if idx is None else np.asarray(idx)
        bad = (ancestors < 0) | (ancestors >= K)
        previous = np.asarray(state[0])[np.arange(B)[:, None], np.where(bad, 0, ancestors)]
        bad = bad | (previous < 0) | (previous >= M)
    bad[:, K - 1] |= outside
    flags = FLAG_INDEX_OUT_OF_RANGE if bad.any() else 0
    return (regime, mean, cov, log_w, flags), errors


def switching_kalman_conditional_step(model, state, idx, uniforms, pinned_regime, y, dtype=np.float64):
    """`switching_kalman_step` with the regime of slot K-1 replaced by pinned_regime [B] (include/aesmc_hip.h:
    aesmc_switching_kalman_conditional_step, K38): slots 0 .. K-2 are that function's, slot K-1 is that function's under
    `_forced` for the pinned regime.  A pinned regime outside [0, M): regime 0, NaN mean, covariance and log-weight for
    slot K-1 and FLAG_INDEX_OUT_OF_RANGE, as a stored regime outside it."""
    with np.errstate(all="ignore"):
        return _conditional_step(model, state, idx, uniforms, pinned_regime, y, dtype, False)[0]


def switching_kalman_conditional_step_bound(model, state, idx, uniforms, pinned_regime, y):
    """`switching_kalman_step_bound` of the conditional step: (bound of mean, of cov, of log_weight)."""
    with np.errstate(all="ignore"):
        _, (mean_e, cov_e, lw_e) = _conditional_step(model, state, idx, uniforms, pinned_regime, y, np.float64, True)
    clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
    return clean(mean_e), clean(cov_e), clean(lw_e)


def conditional_switching_pass(observations, model, num_particles, reference, uniforms, regime_uniforms,
                               ancestor_sampling=True):
    """One whole conditional sweep on replayed uniforms (`aesmc_amd.rao_blackwell.conditional_switching_filter`).
    observations: T x [B,Dy]; model: `operands`' dict; reference: T x int32 [B]; uniforms: T blocks, [B,K] for t <= T-2 (the
    ancestors of step t+1, from step t's weights) and [B,1] for the final draw; regime_uniforms: T x float64 [B,K].

    Backwards first, `switching_information_pass` along the reference (ancestor sampling only); then per step the
    conditional resampling and the conditional Kalman step; then one `categorical_draw` from the last weights and the walk
    back through the ancestors.

    Returns a dict: path (T x int32 [B], the new regime path); regimes, means, covariances, log_weights (T arrays each: the
    stored systems, the reference in slot K-1); ancestral_indices ((T-1) x int64 [B,K]); indices (T x int64 [B], the slot the
    new path passes through); margins (T entries: [B,K] of step t's resampling draws for t <= T-2, [B] of the final draw);
    score_bounds ((T-1) x [B]: the pinned scores' bounds); information ((T-1) tuples or None); flags; and tolerances
    {"means", "covariances", "log_weights"} (T floats each), propagated as `switching_pass` propagates them."""
    T, K = len(observations), int(num_particles)
    B = np.asarray(regime_uniforms[0]).shape[0]
    reference = [np.asarray(r).astype(np.int32) for r in reference]
    with np.errstate(divide="ignore"):
        log_Pi = np.log(model["Pi"])
    flags, information = 0, [None] * (T - 1)
    if ancestor_sampling and T > 1:
        backward = switching_information_pass(model, [r[:, None] for r in reference], observations)
        information, flags = backward["information"], backward["flags"]
    out = {name: [] for name in ("regimes", "means", "covariances", "log_weights", "ancestral_indices", "margins",
                                 "score_bounds")}
    tolerances = {"means": [], "covariances": [], "log_weights": []}
    state, idx = None, None
    for t in range(T):
        if t > 0:
            factor = lam = None
            if ancestor_sampling:
                factor, lam = information[t - 1][3][:, 0, :], information[t - 1][1][:, 0, :]
            idx, bits, margins, bound = switching_conditional_ancestor_index(out["log_weights"][-1], uniforms[t - 1], log_Pi,
                                                                             reference[t], factor, lam, state)
            flags |= bits
            out["ancestral_indices"].append(idx), out["margins"].append(margins), out["score_bounds"].append(bound)
        step_idx = None if idx is None else np.minimum(idx, K - 1)      # (a failed draw is K: the flag says so)
        regime, mean, cov, log_w, bits = switching_kalman_conditional_step(model, state, step_idx, regime_uniforms[t],
                                                                           reference[t], observations[t])
        bound_m, bound_p, bound_w = switching_kalman_conditional_step_bound(model, state, step_idx, regime_uniforms[t],
                                                                            reference[t], observations[t])
        flags |= bits
        D = mean.shape[-1]
        fresh_m = float(np.sqrt((bound_m ** 2).sum(axis=-1)).max())
        fresh_p = float(np.sqrt((unpack(bound_p, D) ** 2).sum(axis=(-2, -1))).max())
        fresh_w = float(bound_w.max())
        if t == 0:
            tol_m, tol_p, tol_w = fresh_m, fresh_p, fresh_w
        else:
            pp, mm, mp, wm, wp = _sensitivities(model, state, step_idx, regime, observations[t])
            before_m, before_p = tolerances["means"][-1], tolerances["covariances"][-1]
            tol_p = 1.01 * pp * before_p + fresh_p
            tol_m = 1.01 * (mm * before_m + mp * before_p) + fresh_m
            tol_w = 1.01 * (wm * before_m + wp * before_p) + fresh_w
        tolerances["means"].append(tol_m), tolerances["covariances"].append(tol_p), tolerances["log_weights"].append(tol_w)
        state = (regime, mean, cov)
        out["regimes"].append(regime), out["means"].append(mean), out["covariances"].append(cov)
        out["log_weights"].append(log_w)
    last, margin, bits = categorical_draw(out["log_weights"][-1], np.asarray(uniforms[T - 1], dtype=np.float64).reshape(B))
    flags |= bits
    out["margins"].append(margin)
    indices, rows = [None] * T, np.arange(B)
    indices[T - 1] = last
    for t in range(T - 2, -1, -1):
        indices[t] = out["ancestral_indices"][t][rows, np.minimum(indices[t + 1], K - 1)]
    out["indices"] = indices
    out["path"] = [out["regimes"][t][rows, np.minimum(indices[t], K - 1)].astype(np.int32) for t in range(T)]
    out.update(information=information, flags=flags, tolerances=tolerances)
    return out


def exact_regime_posterior(model, ys):
    """(sequences [M^T, T] int, probabilities [M^T]) of ONE series (ys: T x [Dy]): the joint law p(s_0..s_{T-1} |
    y_0..y_{T-1}) over all M^T regime sequences by enumeration, each an exact Kalman filter (`_sequence_log_likelihood`) —
    what `exact_regime_marginals` sums per (t, regime)."""
    ys = [np.asarray(y, dtype=np.float64).reshape(1, -1) for y in ys]
    T, M = len(ys), model["A"].shape[0]
    sequences = np.array(list(itertools.product(range(M), repeat=T)), dtype=np.int64)
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    terms = np.empty(len(sequences))
    for position, sequence in enumerate(sequences):
        prior = log_pi0[sequence[0]] + sum(log_Pi[a, b] for a, b in zip(sequence, sequence[1:]))
        terms[position] = prior + _sequence_log_likelihood(model, tuple(int(s) for s in sequence), ys) if np.isfinite(prior) \
            else -np.inf
    weights = np.exp(terms - terms.max())
    return sequences, weights / weights.sum()
