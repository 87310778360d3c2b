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
