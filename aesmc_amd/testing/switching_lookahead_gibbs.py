"""NumPy statement of the CONTRACT of look-ahead particle Gibbs on the regimes of a switching linear-Gaussian model: kernels
K48 (include/aesmc_hip.h: aesmc_switching_lookahead_conditional_ancestor_index and its masked form), K49
(aesmc_switching_kalman_conditional_draw) and the sweep `aesmc_amd.rao_blackwell.conditional_switching_filter(...,
lookahead=True)` makes of them.

There is no new arithmetic here.  Everything is built from `testing.rao_blackwell`'s functions — `switching_lookahead` (K32),
`switching_conditional_ancestor_index` (K37), `_forced` / `_step` (K31), `categorical_draw` (K21) — and the masked forms run
those same functions inside `testing.switching_missing`'s scope.

The sampler.  After a look-ahead draw the K particles of a stored system are EQUALLY weighted.  With the reference path s' in
slot K-1, a step t >= 1 is

    v_j, rows_j   = the look-ahead of stored particle j: log p(y_t | history_j) and the cumulative posterior row
    a_k           ~ Cat(exp v)                                       k = 0 .. K-2: K37's free slots over v
    a_{K-1}       ~ Cat(Pi[s_j, s'_t] x K35's integral of s'_{t..T-1}'s future against N(m_j, P_j))
                                                                     K37's pinned slot over a log-weight of exactly 0.0 —
                                                                     it does NOT carry v_j: the weights that enter ancestor
                                                                     sampling are those of system t-1, which are equal
                    (without ancestor sampling a_{K-1} = K-1)
    s_t^k         ~ rows_{a_k}   k = 0 .. K-2;     s_t^{K-1} = s'_t;     then the Kalman update through the ancestors

and the path is one draw from EQUAL weights at the end, walked back through the ancestors.

(This package never imports the oracle — tests/test_library.py.)
"""
import contextlib

import numpy as np

from . import rao_blackwell as rb
from . import switching_missing as missing


def _scope(y, observed):
    """(the scope the functions of `testing.rao_blackwell` run in, the observation they take): with a mask,
    `switching_missing`'s scope and the marked observation."""
    if observed is None:
        return contextlib.nullcontext(), np.asarray(y)
    return missing._masked(), missing.mark(y, observed)


def _index(model, log_Pi, state, y, u, regime_next, factor, lam):
    log_w, cdf, flags = rb.switching_lookahead(model, log_Pi, state, y)
    bounds = rb.switching_lookahead_bound(model, log_Pi, state, y)
    K = log_w.shape[1]
    idx, bits, margins, _ = rb.switching_conditional_ancestor_index(log_w, u, None, None, None, None, None)
    flags |= bits
    score_bound = np.zeros(log_w.shape[0])
    if factor is not None or lam is not None:
        pinned, bits, pinned_margins, score_bound = rb.switching_conditional_ancestor_index(
            np.zeros_like(log_w), u, log_Pi, regime_next, factor, lam, state)
        flags |= bits
        good = idx[:, K - 1] == K - 1      # (K where the row's first-stage weights are bad: every slot stays K)
        idx[:, K - 1] = np.where(good, pinned[:, K - 1], K)
        margins[:, K - 1] = np.where(good, pinned_margins[:, K - 1], np.inf)
    return idx, log_w, cdf, flags, margins, score_bound, bounds


def lookahead_conditional_ancestor_index(model, log_Pi, state, y, u, regime_next, factor, lam, observed=None):
    """(idx int64 [B,K], log_weight [B,K], cdf [B,K,M], flags, margins [B,K], score_bound [B], lookahead_bounds) of the
    resampling side of one look-ahead conditional step (K48; with `observed` bool [B,Dy] its masked form).

    model: `operands`' dict; log_Pi [M,M]; state: the stored (regime, mean, cov); y [B,Dy]; u [B,K]; regime_next int32 [B];
    factor [B,D(D+1)/2], lam [B,D] or both None (no ancestor sampling).  By definition

        log_weight, cdf = switching_lookahead(model, log_Pi, state, y)
        idx[:, :K-1]    = switching_conditional_ancestor_index(log_weight, u, None, None, None, None, None)[:, :K-1]
        idx[:, K-1]     = switching_conditional_ancestor_index(zeros, u, log_Pi, regime_next, factor, lam, state)[:, K-1]
                          (K-1 without ancestor sampling; K where the first call marks the row bad)

    flags: the three calls' together.  margins: `_step_margins` of every draw; score_bound: the pinned scores' bound;
    lookahead_bounds: `switching_lookahead_bound`'s (of log_weight, of cdf)."""
    scope, y = _scope(y, observed)
    with scope:
        return _index(model, log_Pi, state, y, u, regime_next, factor, lam)


def _conditional_draw(model, state, idx, uniforms, cdf, pinned_regime, y, dtype, track):
    uniforms = np.asarray(uniforms, dtype=np.float64)
    B, K = uniforms.shape
    M = model["A"].shape[0]
    rows = np.asarray(cdf, dtype=np.float64)
    if state is not None and idx is not None:
        idx = np.asarray(idx)
        rows = rows[np.arange(B)[:, None], np.where((idx < 0) | (idx >= K), 0, idx)]
    s = (rows[:, :, :M - 1] <= uniforms[:, :, None]).sum(axis=2)      # (a NaN row: regime 0)
    pinned_regime = np.asarray(pinned_regime)
    outside = (pinned_regime < 0) | (pinned_regime >= M)
    s[:, K - 1] = np.where(outside, 0, pinned_regime)
    shim, forced = rb._forced(model, s)
    (regime, mean, cov, ell, flags), errors = rb._step(shim, state, idx, forced, y, dtype, track)
    regime, mean, cov, ell = regime.copy(), mean.copy(), cov.copy(), ell.copy()
    regime[outside, K - 1], mean[outside, K - 1], cov[outside, K - 1], ell[outside, K - 1] = 0, np.nan, np.nan, np.nan
    if track:
        for e in errors:
            e[outside, K - 1] = 0.0
    if outside.any():
        flags |= rb.FLAG_INDEX_OUT_OF_RANGE
    return (regime, mean, cov, ell, flags), errors, rows


def switching_kalman_conditional_draw(model, state, idx, uniforms, cdf, pinned_regime, y, observed=None, dtype=np.float64):
    """(regime int32 [B,K], mean, cov, log_likelihood [B,K], flags) of K49: `switching_kalman_draw` — the regime of slot k
    from the ancestor's row of cdf [B,K,M] — with slot K-1's regime replaced by pinned_regime [B], as
    `switching_kalman_conditional_step` replaces it: `_step` under `_forced`.  A pinned regime outside [0, M): regime 0, NaN
    mean, covariance and log-likelihood for slot K-1 and FLAG_INDEX_OUT_OF_RANGE."""
    scope, y = _scope(y, observed)
    with scope, np.errstate(all="ignore"):
        return _conditional_draw(model, state, idx, uniforms, cdf, pinned_regime, y, dtype, False)[0]


def switching_kalman_conditional_draw_bound(model, state, idx, uniforms, cdf, pinned_regime, y, observed=None):
    """`switching_kalman_step_bound` of that step: (bound of mean, of cov, of log_likelihood)."""
    scope, y = _scope(y, observed)
    with scope, np.errstate(all="ignore"):
        _, (mean_e, cov_e, ll_e), _ = _conditional_draw(model, state, idx, uniforms, cdf, pinned_regime, y, np.float64, True)
    clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
    return clean(mean_e), clean(cov_e), clean(ll_e)


def _pass(observations, model, num_particles, reference, uniforms, regime_uniforms, ancestor_sampling):
    T, K = len(observations), int(num_particles)
    B = np.asarray(regime_uniforms[0]).shape[0]
    M = model["A"].shape[0]
    reference = [np.asarray(r).astype(np.int32) for r in reference]
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    flags, information = 0, [None] * (T - 1)
    if ancestor_sampling and T > 1:
        backward = rb.switching_information_pass(model, [r[:, None] for r in reference], observations)
        information, flags = backward["information"], backward["flags"]
    out = {name: [] for name in ("regimes", "means", "covariances", "first_stage_log_weights", "ancestral_indices", "margins",
                                 "regime_margins", "score_bounds")}
    tolerances = {name: [] for name in ("means", "covariances", "first_stage_log_weights", "cdf")}
    state, idx = None, None
    for t in range(T):
        y = observations[t]
        carried = 0.0
        if t == 0:
            log_v, cdf, bits = rb.switching_lookahead(model, log_pi0, None, y, K)
            bound_v, bound_c = rb.switching_lookahead_bound(model, log_pi0, None, y, K)
        else:
            factor = lam = None
            if ancestor_sampling:
                factor, lam = information[t - 1][3][:, 0, :], information[t - 1][1][:, 0, :]
            idx, log_v, cdf, bits, margins, bound, (bound_v, bound_c) = _index(model, log_Pi, state, y, uniforms[t - 1],
                                                                               reference[t], factor, lam)
            out["ancestral_indices"].append(idx), out["margins"].append(margins), out["score_bounds"].append(bound)
            before_m, before_p = tolerances["means"][-1], tolerances["covariances"][-1]
            rows = log_Pi[np.clip(state[0], 0, M - 1)]
            for j in range(M):      # (as `adapted_switching_pass`: what the input state's error does to a score)
                considered = np.where(np.isneginf(rows[:, :, j]), np.argmax(rows, axis=-1), j)
                _, _, _, wm, wp = rb._sensitivities(model, state, None, considered, y)
                carried = max(carried, 1.01 * (wm * before_m + wp * before_p))
        flags |= bits
        tolerances["first_stage_log_weights"].append(carried + float(bound_v.max()))
        tolerances["cdf"].append(carried + float(bound_c.max()))
        step_idx = None if idx is None else np.minimum(idx, K - 1)      # (a failed draw is K: the flag says so)
        with np.errstate(all="ignore"):
            (regime, mean, cov, _, bits), (bound_m, bound_p, _), rows = _conditional_draw(
                model, state, step_idx, regime_uniforms[t], cdf, reference[t], y, np.float64, True)
        flags |= bits
        out["regime_margins"].append(rb._regime_margin(rows[:, :K - 1], np.asarray(regime_uniforms[t])[:, :K - 1]))
        D = mean.shape[-1]
        clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
        fresh_m = float(np.sqrt((clean(bound_m) ** 2).sum(axis=-1)).max())
        fresh_p = float(np.sqrt((rb.unpack(clean(bound_p), D) ** 2).sum(axis=(-2, -1))).max())
        if t == 0:
            tol_m, tol_p = fresh_m, fresh_p
        else:
            pp, mm, mp, _, _ = rb._sensitivities(model, state, step_idx, regime, y)
            tol_p = 1.01 * pp * before_p + fresh_p
            tol_m = 1.01 * (mm * before_m + mp * before_p) + fresh_m
        tolerances["means"].append(tol_m), tolerances["covariances"].append(tol_p)
        state = (regime, mean, cov)
        out["regimes"].append(regime), out["means"].append(mean), out["covariances"].append(cov)
        out["first_stage_log_weights"].append(log_v)
    last, margin, bits = rb.categorical_draw(np.zeros((B, K)), np.asarray(uniforms[T - 1], dtype=np.float64).reshape(B))
    flags |= bits
    out["margins"].append(margin)
    indices, rows = [None] * T, np.arange(B)
    indices[T - 1] = last
    for t in range(T - 2, -1, -1):
        indices[t] = out["ancestral_indices"][t][rows, np.minimum(indices[t + 1], K - 1)]
    out["indices"] = indices
    out["path"] = [out["regimes"][t][rows, np.minimum(indices[t], K - 1)].astype(np.int32) for t in range(T)]
    out["log_weights"] = [np.zeros((B, K)) for _ in range(T)]
    out.update(information=information, flags=flags, tolerances=tolerances)
    return out


def lookahead_conditional_switching_pass(observations, model, num_particles, reference, uniforms, regime_uniforms,
                                         ancestor_sampling=True, observed=None):
    """One whole look-ahead conditional sweep on replayed uniforms (`conditional_switching_filter(..., lookahead=True)`).
    Arguments as `testing.rao_blackwell.conditional_switching_pass`'s; observed: None, or T entries of None or bool [B,Dy].

    Backwards first, `switching_information_pass` along the reference (ancestor sampling only).  Step 0: the look-ahead on
    the prior and the conditional draw.  Step t >= 1: `lookahead_conditional_ancestor_index` on stored system t-1 and the
    conditional draw through its ancestors.  Then one `categorical_draw` from EQUAL weights and the walk back.

    Returns a dict: path (T x int32 [B]); regimes, means, covariances (T arrays each: the stored, equally weighted systems,
    the reference in slot K-1); log_weights (T zero arrays); first_stage_log_weights (T x [B,K]; step 0's on the prior);
    ancestral_indices ((T-1) x int64 [B,K]); indices (T x int64 [B]); margins (T entries: [B,K] of step t's resampling draws
    for t <= T-2, [B] of the final draw); regime_margins (T floats: `_regime_margin` of the free slots' regime draws);
    score_bounds ((T-1) x [B]); information; flags; and tolerances {"means", "covariances", "first_stage_log_weights",
    "cdf"} (T floats each), propagated as `adapted_switching_pass` propagates its own."""
    if observed is None:
        return _pass(observations, model, num_particles, reference, uniforms, regime_uniforms, ancestor_sampling)
    with missing._masked():
        return _pass(missing._marked(observations, observed), model, num_particles, reference, uniforms, regime_uniforms,
                     ancestor_sampling)
