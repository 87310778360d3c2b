"""NumPy statement of the CONTRACT of the collapsed-mixture filter and smoother of a switching linear-Gaussian model (GPB2,
which is Kim's filter — Kim 1994; Kim & Nelson 1999 — and its first-order cousin IMM, Blom & Bar-Shalom 1988): the two
kernels K50 and K51 (include/aesmc_hip.h: aesmc_switching_collapse, aesmc_switching_pair_smooth) with the bounds they are held
to, and the passes that `aesmc_amd.rao_blackwell.collapsed_switching_filter` and `collapsed_switching_smooth` make of K31
with the regime forced and those two.  Written without regard to the kernels' structure (no padding, no LDS).

The collapse of group (b,g), N components (lw_n, m_n, P_n); every sum ascending in n from the value named first, every
product rounded before it is added (the kernel fuses them: `switching_collapse_bound`):

    top = max_n lw_n;   e_n = exp(lw_n - top);   sum = 0 + sum_n e_n;   log_mass = top + log(sum);   w_n = e_n (1 / sum)
    mean_p = 0 + sum_n w_n m_np;      cov_ps = 0 + sum_n [w_n P_n,ps, then (w_n d_np) d_ns],  d_n = m_n - mean

A group of weights all -inf: log_mass -inf, zero mean, zero covariance.  A component of weight -inf enters no chain (its
moments may be NaN).  A NaN weight: NaN outputs for the group.

The pair step (b,i,j): component i filtered at t, N(m, P), against regime j's smoothed component of t+1, N(ms, Ps) —
`testing.switching_state_draw`'s measurement update (V, e, S, L, v, U under the same dropping rule) and then

    X_il = (Ps_il - sum_{c<i} L_ic X_cl) rk_i;      Gm_ik = (X_ik - sum_{c<k} Gm_ic L_kc) rk_k;      Y_ks = 0 + sum_c Gm_kc U_cs
    m'_p = m_p + sum_i U_ip v_i;      P'_ps = P_ps - sum_k U_kp U_ks + sum_k U_kp Y_ks

which is the Rauch-Tung-Striebel step m' = m + J (ms - A m - b), P' = P + J (Ps - S) J^T with J = P A^T S^-1.

The passes.  Per batch row the state is M components (log mu_i, m_i, P_i), mu_i = p(s_t = i | y_{0:t}); everything in the
log domain; a score whose prior part is -inf is -inf whatever its likelihood part is (K32's rule):

    step 0        K31's step-0 form on M slots, slot j forced to regime j: (m_j, P_j, l_j);  g_j = log pi0_j + l_j
    order 2, t>0  K31 forced on M^2 slots, slot j M + i from component i under regime j: l_ij;
                  g[b,j,i] = (log mu_i + log Pi[i,j]) + l_ij;  the collapse of group j over i: (mass_j, m_j, P_j);  g_j = mass_j
    order 1, t>0  the collapse, shared components, under the weights log mu_i + log Pi[i,j]: (log c_j, m0_j, P0_j); K31 forced
                  on M slots from those: (m_j, P_j, l_j);  g_j = log c_j + l_j
    every step    the collapse of the one group of the M components under g: its mass is the evidence increment lse_j g_j, its
                  mean and covariance the filtered ones;  log mu_j = g_j - increment
    smoother      at T-1 the filtered quantities; for t = T-2 .. 0:
                  log joint[b,i,j] = (g_{t+1}[b,j,i] - mass_{t+1}[b,j]) + log mu^s_{t+1}[b,j]  (-inf where the last is -inf),
                  the pair step for every (i,j), the collapse of group i over j under log joint[b,i,:]: its mass is
                  log mu^s_t(i); then the one group of the M smoothed components under log mu^s_t: the smoothed moments

(This package never imports the oracle — tests/test_library.py.)
"""
import contextlib

import numpy as np

from . import rao_blackwell as rb
from . import switching_missing as missing
from . import switching_state_draw as draw

MAX_COMPONENTS, MAX_GROUPS = 256, 256
# (B, G, N, D) of K50: one lane; two groups of two; an odd N at the largest D; D between two padded extents; the largest N,
# several groups; several workgroups with a partial last one
COLLAPSE_SHAPES = [(1, 1, 1, 1), (3, 2, 2, 2), (2, 3, 9, 8), (2, 4, 16, 5), (1, 16, 256, 8), (300, 2, 2, 3)]
# (B, M, D, Dy) of K51: K31's step shapes without the particles; the last one spans two workgroups with a partial last one
PAIR_SHAPES = [(1, 1, 1, 1), (3, 2, 2, 1), (2, 3, 8, 8), (2, 4, 5, 3), (1, 16, 8, 1), (70, 2, 3, 2)]


# ---- K50 -------------------------------------------------------------------------------------------------------------------------
def _collapse(mean, cov, log_weight, dtype, track):
    """The collapse on (value, error) pairs; `track` false: plain values.  Returns ((log_mass, mean, cov), (errors of the
    three))."""
    tri = rb.tri
    lw = np.asarray(log_weight, dtype=np.float64)
    B, G, N = lw.shape
    mean, cov = np.asarray(mean), np.asarray(cov)
    if mean.ndim == 3:      # the shared-components form
        mean, cov = mean[:, None], cov[:, None]
    D = mean.shape[-1]
    TD = D * (D + 1) // 2
    mean, cov = np.broadcast_to(mean, (B, G, N, D)), np.broadcast_to(cov, (B, G, N, TD))
    zero = np.zeros((B, G), dtype=dtype)
    given = lambda array: (np.asarray(array).astype(dtype), zero if track else None)
    one = given(zero + 1.0)
    bad = np.isnan(lw).any(axis=2)
    top = np.where(bad, np.nan, lw.max(axis=2, initial=-np.inf))
    empty = ~bad & np.isneginf(top)
    skip = np.isneginf(lw)                                              # [B,G,N]
    safe_top = np.where(empty | bad, 0.0, top)
    drop = lambda pair, n: (np.where(skip[:, :, n], 0.0, pair[0]), None if not track else np.where(skip[:, :, n], 0.0, pair[1]))
    e = [rb._exp(rb._minus(given(lw[:, :, n]), given(safe_top))) for n in range(N)]
    total = rb._chain(given(zero), [(e[n], one) for n in range(N)])
    log_mass = rb._chain(given(safe_top), [(rb._log(total), one)])
    scale = rb._reciprocal(total)
    w = [drop(rb._times(e[n], scale), n) for n in range(N)]
    # (a skipped component's moments are replaced by zeros: its terms add 0 and nothing to the bound)
    m = [[drop(given(mean[:, :, n, p]), n) for p in range(D)] for n in range(N)]
    P = [[drop(given(cov[:, :, n, c]), n) for c in range(TD)] for n in range(N)]
    centre = [rb._chain(given(zero), [(w[n], m[n][p]) for n in range(N)]) for p in range(D)]
    d = [[drop(rb._minus(m[n][p], centre[p]), n) for p in range(D)] for n in range(N)]
    spread = []
    for p in range(D):
        wd = [rb._times(w[n], d[n][p]) for n in range(N)]
        for s in range(p + 1):
            terms = []
            for n in range(N):
                terms += [(w[n], P[n][tri(p, s)]), (wd[n], d[n][s])]
            spread.append(rb._chain(given(zero), terms))

    def finish(parts, hollow):
        values = np.stack([part[0] for part in parts], axis=-1)
        values[empty] = hollow
        values[bad] = np.nan
        errors = None
        if track:
            errors = np.stack([part[1] for part in parts], axis=-1).astype(np.float64)
            errors[empty | bad | np.isnan(values).any(axis=-1)] = 0.0
        return values, errors

    (mass_v, mass_e), (mean_v, mean_e), (cov_v, cov_e) = finish([log_mass], -np.inf), finish(centre, 0.0), finish(spread, 0.0)
    return (mass_v[..., 0], mean_v, cov_v), (None if mass_e is None else mass_e[..., 0], mean_e, cov_e)


def switching_collapse(mean, cov, log_weight, dtype=np.float64):
    """(log_mass [B,G], mean [B,G,D], cov [B,G,D(D+1)/2]) of the moment-matching collapse (include/aesmc_hip.h:
    aesmc_switching_collapse) — the module docstring states the arithmetic.

    mean [B,G,N,D] and cov [B,G,N,D(D+1)/2] (packed lower triangles), or [B,N,D] and [B,N,D(D+1)/2]: the row's components
    shared by its G groups; log_weight [B,G,N]; dtype: the arithmetic (np.float64: the contract; np.longdouble: what the
    bound is checked against)."""
    with np.errstate(all="ignore"):
        return _collapse(mean, cov, log_weight, dtype, False)[0]


def switching_collapse_bound(mean, cov, log_weight):
    """(bound of log_mass [B,G], of mean [B,G,D], of cov [B,G,D(D+1)/2]), float64: `testing.rao_blackwell.
    switching_kalman_step_bound`'s running error analysis of the collapse — `_chain`, `_times`, `_reciprocal`, `_log`,
    `_exp`, `_minus`; 2 * 1.01 times the running bound: two evaluations, each within it of the exact value.  The inputs
    enter exactly.  Zero where the output is NaN and for an empty group (exact on both sides)."""
    with np.errstate(all="ignore"):
        _, errors = _collapse(mean, cov, log_weight, np.float64, True)
    return tuple(np.where(np.isfinite(e), 2 * 1.01 * e, np.inf) for e in errors)


def example_collapse(B, G, N, D, seed=0):
    """(mean [B,G,N,D], cov [B,G,N,D(D+1)/2], log_weight [B,G,N]) of one collapse: standard-normal means, covariances
    F F^T / D + 0.1 I, log-weights 2 N(0,1) (a spread of weights over several orders of magnitude)."""
    rng = np.random.default_rng([seed, B, G, N, D, 50])
    factor = rng.standard_normal((B, G, N, D, D))
    cov = rb.pack(factor @ np.swapaxes(factor, -1, -2) / D + 0.1 * np.eye(D))
    return rng.standard_normal((B, G, N, D)), np.ascontiguousarray(cov), 2.0 * rng.standard_normal((B, G, N))


# ---- K51 -------------------------------------------------------------------------------------------------------------------------
def _pair(model, mean, cov, mean_next, cov_next, dtype, track):
    """The pair step on (value, error) pairs.  Returns ((means [B,M,M,D], covs [B,M,M,TD], margin), (their errors,
    clearance))."""
    tri = rb.tri
    mean, cov, mean_next, cov_next = (np.asarray(x) for x in (mean, cov, mean_next, cov_next))
    B, M, D = mean.shape
    TD = D * (D + 1) // 2
    shape = (B, M, M)
    zero = np.zeros(shape, dtype=dtype)
    given = lambda array: (np.broadcast_to(np.asarray(array), shape).astype(dtype), zero if track else None)
    m = [given(mean[:, :, None, i]) for i in range(D)]
    P = [given(cov[:, :, None, e]) for e in range(TD)]
    ms = [mean_next[:, None, :, i] for i in range(D)]
    Ps = [given(cov_next[:, None, :, e]) for e in range(TD)]
    A, bb, q = model["A"][None, None], model["b"][None, None], model["q"][None, None]      # [1,1,M(j),...]
    Am = [[given(A[:, :, :, i, l]) for l in range(D)] for i in range(D)]
    V = [[rb._chain(given(zero), [(Am[i][c], P[tri(c, l)]) for c in range(D)]) for l in range(D)] for i in range(D)]
    e = [rb._chain(given(ms[i] - bb[:, :, :, i]), [(Am[i][l], m[l]) for l in range(D)], negate=True) for i in range(D)]
    S = {}
    for i in range(D):
        for k in range(i + 1):
            start = given(q[:, :, :, i] * q[:, :, :, i]) if i == k else given(zero)
            S[tri(i, k)] = rb._chain(start, [(Am[i][l], V[k][l]) for l in range(D)])
    top = S[0][0]
    for i in range(1, D):
        top = np.maximum(top, S[tri(i, i)][0])
    top_error = np.maximum.reduce([S[tri(i, i)][1] for i in range(D)]) if track else None
    L, rk, kept, margin, clearance = draw._factor(S, D, top, top_error, dtype, track)
    keep = lambda pair, i: (np.where(kept[i], pair[0], 0.0), None if not track else np.where(kept[i], pair[1], 0.0))
    v, U, X = [], [], []
    for i in range(D):
        v.append(keep(rb._times(rb._chain(e[i], [(L[tri(i, c)], v[c]) for c in range(i)], negate=True), rk[i]), i))
        U.append([keep(rb._times(rb._chain(V[i][l], [(L[tri(i, c)], U[c][l]) for c in range(i)], negate=True), rk[i]), i)
                  for l in range(D)])
        X.append([keep(rb._times(rb._chain(Ps[tri(i, l)], [(L[tri(i, c)], X[c][l]) for c in range(i)], negate=True), rk[i]), i)
                  for l in range(D)])
    Gm = []
    for i in range(D):
        row = []
        for k in range(D):
            row.append(keep(rb._times(rb._chain(X[i][k], [(row[c], L[tri(k, c)]) for c in range(k)], negate=True), rk[k]), k))
        Gm.append(row)
    Y = [[rb._chain(given(zero), [(Gm[k][c], U[c][s]) for c in range(D)]) for s in range(D)] for k in range(D)]
    mp = [rb._chain(m[p], [(U[i][p], v[i]) for i in range(D)]) for p in range(D)]
    Pp = [rb._chain(rb._chain(P[tri(p, s)], [(U[k][p], U[k][s]) for k in range(D)], negate=True),
                    [(U[k][p], Y[k][s]) for k in range(D)]) for p in range(D) for s in range(p + 1)]

    def finish(parts):
        values = np.stack([part[0] for part in parts], axis=-1)
        errors = None
        if track:
            errors = np.stack([part[1] for part in parts], axis=-1).astype(np.float64)
            errors[np.isnan(values).any(axis=-1)] = 0.0      # (a NaN handed in stays one: nothing to bound)
        return values, errors

    (mean_v, mean_e), (cov_v, cov_e) = finish(mp), finish(Pp)
    smallest = lambda array: float(array.min()) if array.size else float("inf")
    return (mean_v, cov_v, smallest(margin)), (mean_e, cov_e, smallest(clearance))


def switching_pair_smooth(model, mean, cov, mean_next, cov_next, dtype=np.float64):
    """(means [B,M,M,D], covs [B,M,M,D(D+1)/2], margin) of the Rauch-Tung-Striebel step between components
    (include/aesmc_hip.h: aesmc_switching_pair_smooth): entry (b,i,j) is component i of (mean [B,M,D], cov [B,M,D(D+1)/2]),
    filtered at t, smoothed against component j of (mean_next, cov_next), smoothed at t+1, through A_j, b_j, q_j of
    `model` (`testing.rao_blackwell.operands`' dict).  `margin`: the smallest |pivot - threshold| / (the largest diagonal
    entry of S) over all pairs, as `testing.switching_state_draw.state_draw_step`'s."""
    with np.errstate(all="ignore"):
        return _pair(model, mean, cov, mean_next, cov_next, dtype, False)[0]


def switching_pair_smooth_bound(model, mean, cov, mean_next, cov_next):
    """(bound of means, bound of covs, clearance): the running error analysis of the pair step (`_chain`, `_times`, `_sqrt`,
    `_reciprocal`; 2 * 1.01 times the running bound; the inputs enter exactly).  The bound holds for a device that keeps
    and drops the same pivots, which it does when `clearance` (`state_draw_step_bound`'s) exceeds 1."""
    with np.errstate(all="ignore"):
        _, (mean_e, cov_e, clearance) = _pair(model, mean, cov, mean_next, cov_next, np.float64, True)
    clean = lambda errors: np.where(np.isfinite(errors), 2 * 1.01 * errors, np.inf)
    return clean(mean_e), clean(cov_e), clearance


def example_pair_smooth(B, M, D, Dy, seed=0):
    """(model, mean, cov, mean_next, cov_next) of one pair step: `example_model` and two sets of components as
    `example_step`'s state."""
    rng = np.random.default_rng([seed, B, M, D, Dy, 51])
    model = rb.example_model(M, D, Dy, seed)

    def components():
        factor = rng.standard_normal((B, M, D, D))
        return rng.standard_normal((B, M, D)), np.ascontiguousarray(rb.pack(factor @ np.swapaxes(factor, -1, -2) / D +
                                                                            0.1 * np.eye(D)))
    return (model,) + components() + components()


# ---- the passes --------------------------------------------------------------------------------------------------------------------
def _scored(prior, likelihood):
    """prior + likelihood; -inf where the prior is -inf whatever the likelihood is (K32's rule)."""
    with np.errstate(all="ignore"):
        return np.where(np.isneginf(prior), -np.inf, prior + likelihood)


def collapsed_pass(observations, model, order=2, observed=None):
    """The collapsed-mixture filter (order 2: GPB2 / Kim's filter; order 1: IMM) — the module docstring states the steps.
    observations: T x [B,Dy]; model: `operands`' dict; observed: None, or T entries of None or bool [B,Dy].

    Returns a dict: log_marginal_likelihood [B] (the increments summed in time order), log_regime_probabilities (T x [B,M]),
    means (T x [B,M,D]), covariances (T x [B,M,D(D+1)/2]), regime_probabilities [T,B,M], filtered_mean [T,B,D],
    filtered_covariance [T,B,D,D], flags, and what the smoother reads: scores (T entries: None, then g_t [B,M,M] indexed
    (b,j,i); order 2 only) and masses (T entries: None, then [B,M])."""
    if order not in (1, 2):
        raise ValueError("collapsed_pass: order must be 1 or 2")
    T = len(observations)
    M, D = model["A"].shape[0], model["A"].shape[-1]
    TD = D * (D + 1) // 2
    B = np.asarray(observations[0]).shape[0]
    marked = missing._marked(observations, observed)
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    slots = np.ascontiguousarray(np.broadcast_to(np.arange(M, dtype=np.int32), (B, M)))
    pair_regime = np.repeat(slots, M, axis=1)                          # slot j M + i: regime j
    out = {name: [] for name in ("log_regime_probabilities", "means", "covariances", "scores", "masses")}
    overall_mean, overall_cov = [], []
    total, flags, log_mu, mean, cov = np.zeros(B), 0, None, None, None
    with missing._masked() if observed is not None else contextlib.nullcontext():
        for t in range(T):
            scores = mass = None
            if t == 0:
                shim, forced = rb._forced(model, slots)
                _, mean, cov, likelihood, bits = rb.switching_kalman_step(shim, None, None, forced, marked[0])
                g = _scored(np.broadcast_to(log_pi0, (B, M)), likelihood)
            else:
                prior = log_mu[:, None, :] + log_Pi.T[None]            # [b,j,i] = log mu_i + log Pi[i,j]
                if order == 2:
                    shim, forced = rb._forced(model, pair_regime)
                    state = (np.tile(slots, (1, M)), np.tile(mean, (1, M, 1)), np.tile(cov, (1, M, 1)))      # slot j M + i: component i
                    _, pair_mean, pair_cov, likelihood, bits = rb.switching_kalman_step(shim, state, None, forced, marked[t])
                    scores = _scored(prior, likelihood.reshape(B, M, M))
                    mass, mean, cov = switching_collapse(pair_mean.reshape(B, M, M, D), pair_cov.reshape(B, M, M, TD), scores)
                    g = mass
                else:
                    mass, mixed_mean, mixed_cov = switching_collapse(mean, cov, prior)
                    shim, forced = rb._forced(model, slots)
                    _, mean, cov, likelihood, bits = rb.switching_kalman_step(shim, (slots, mixed_mean, mixed_cov), None, forced,
                                                                              marked[t])
                    g = _scored(mass, likelihood)
            flags |= bits
            increment, centre, spread = switching_collapse(mean[:, None], cov[:, None], g[:, None, :])
            with np.errstate(invalid="ignore"):
                log_mu = g - increment
            total = total + increment[:, 0]
            out["log_regime_probabilities"].append(log_mu), out["means"].append(mean), out["covariances"].append(cov)
            out["scores"].append(scores), out["masses"].append(mass)
            overall_mean.append(centre[:, 0]), overall_cov.append(rb.unpack(spread[:, 0], D))
    out.update(log_marginal_likelihood=total, flags=flags, regime_probabilities=np.exp(np.stack(out["log_regime_probabilities"])),
               filtered_mean=np.stack(overall_mean), filtered_covariance=np.stack(overall_cov))
    return out


def collapsed_smooth_pass(observations, model, observed=None):
    """The collapsed-mixture smoother (Kim 1994): `collapsed_pass` of order 2, then the backward pass of the module docstring.

    Returns `collapsed_pass`'s dict and smoothed_log_regime_probabilities (T x [B,M]), smoothed_means (T x [B,M,D]),
    smoothed_covariances (T x [B,M,D(D+1)/2]), smoothed_regime_probabilities [T,B,M], smoothed_pair_probabilities [T-1,B,M,M]
    (p(s_t = i, s_{t+1} = j | y), indexed (b,i,j)), smoothed_mean [T,B,D], smoothed_covariance [T,B,D,D], margin (the smallest
    over the pair steps)."""
    out = collapsed_pass(observations, model, 2, observed)
    T = len(observations)
    D = model["A"].shape[-1]
    B, M = out["log_regime_probabilities"][0].shape
    log_s, means, covs = [None] * T, [None] * T, [None] * T
    pairs, centre, spread = [None] * (T - 1), [None] * T, [None] * T
    log_s[T - 1], means[T - 1], covs[T - 1] = out["log_regime_probabilities"][T - 1], out["means"][T - 1], out["covariances"][T - 1]
    centre[T - 1], spread[T - 1] = out["filtered_mean"][T - 1], out["filtered_covariance"][T - 1]
    margin = float("inf")
    for t in range(T - 2, -1, -1):
        with np.errstate(invalid="ignore"):
            conditional = np.swapaxes(out["scores"][t + 1] - out["masses"][t + 1][:, :, None], 1, 2)      # [b,i,j]
        joint = _scored(np.broadcast_to(log_s[t + 1][:, None, :], (B, M, M)), conditional)
        pair_mean, pair_cov, step_margin = switching_pair_smooth(model, out["means"][t], out["covariances"][t], means[t + 1],
                                                                 covs[t + 1])
        margin = min(margin, step_margin)
        log_s[t], means[t], covs[t] = switching_collapse(pair_mean, pair_cov, joint)
        _, overall_mean, overall_cov = switching_collapse(means[t][:, None], covs[t][:, None], log_s[t][:, None, :])
        pairs[t], centre[t], spread[t] = np.exp(joint), overall_mean[:, 0], rb.unpack(overall_cov[:, 0], D)
    out.update(smoothed_log_regime_probabilities=log_s, smoothed_means=means, smoothed_covariances=covs,
               smoothed_regime_probabilities=np.exp(np.stack(log_s)),
               smoothed_pair_probabilities=np.stack(pairs) if T > 1 else np.zeros((0, B, M, M)),
               smoothed_mean=np.stack(centre), smoothed_covariance=np.stack(spread), margin=margin)
    return out
