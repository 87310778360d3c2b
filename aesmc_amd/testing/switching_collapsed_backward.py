"""The CONTRACT of the differentiable collapsed-mixture evidence of a switching linear-Gaussian model: NumPy statements of
the adjoint kernels K52 / K53 (include/aesmc_hip.h: aesmc_switching_kalman_step_backward and its masked form) and K54
(aesmc_switching_collapse_backward), and `collapsed_log_likelihood_restated`, the whole differentiable pass of
`aesmc_amd.rao_blackwell.collapsed_switching_log_likelihood` in plain torch float64 — dense covariances,
torch.linalg.cholesky / solve_triangular, deleted rows for the mask; no kernels and no packed layout, so it shares nothing
with what it checks.

The NumPy statements are written on full matrices without regard to the kernels' structure (no padding, no LDS, no
workspace); `dtype` is the arithmetic (np.float64: the contract; np.longdouble: what the inputs' conditioning is checked
against).  Packed covariances: the gradient with respect to a packed element is the derivative of the function of the
packed vector — an off-diagonal element stands for both symmetric positions — which is what autograd through
`rao_blackwell.unpack_covariance` gives.

(This package never imports the oracle — tests/test_library.py.)
"""
import math

import numpy as np
import torch

from . import rao_blackwell as rb

PARAMETERS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
# (B, slots, M, D, Dy) of K52 / K53: every pair of padded extents (2, 4, 8) at least once; the last spans two 256-lane
# workgroups (several 64-lane ones where an extent is 8: (2, 9, 3, 8, 8) and (1, 16, 16, 8, 1) have partial ones)
STEP_SHAPES = [(1, 1, 1, 1, 1), (3, 4, 2, 2, 1), (2, 4, 2, 2, 3), (2, 4, 2, 1, 8), (2, 9, 3, 4, 2), (2, 9, 3, 3, 4),
               (2, 4, 2, 4, 7), (2, 4, 2, 8, 2), (2, 4, 2, 7, 3), (2, 9, 3, 8, 8), (1, 16, 16, 8, 1), (70, 4, 2, 3, 2)]
STEP_OUTPUTS = ("grad_mean_in", "grad_cov_in", "grad_m0", "grad_s0", "grad_A", "grad_b", "grad_q", "grad_C", "grad_d", "grad_r")


# ---- small dense algebra in any dtype (np.linalg has no extended precision) -------------------------------------------------------
def _cholesky(S):
    n = S.shape[-1]
    L = np.zeros_like(S)
    for j in range(n):
        pivot = S[..., j, j] - (L[..., j, :j] ** 2).sum(axis=-1)
        L[..., j, j] = np.sqrt(pivot)
        for i in range(j + 1, n):
            L[..., i, j] = (S[..., i, j] - (L[..., i, :j] * L[..., j, :j]).sum(axis=-1)) / L[..., j, j]
    return L


def _solve_lower(L, X):
    """L^-1 X."""
    out = np.zeros_like(X)
    for i in range(L.shape[-1]):
        out[..., i, :] = (X[..., i, :] - (L[..., i, :i, None] * out[..., :i, :]).sum(axis=-2)) / L[..., i, i, None]
    return out


def _solve_upper(L, X):
    """L^-T X."""
    n = L.shape[-1]
    out = np.zeros_like(X)
    for i in range(n - 1, -1, -1):
        out[..., i, :] = (X[..., i, :] - (L[..., i + 1:, i, None] * out[..., i + 1:, :]).sum(axis=-2)) / L[..., i, i, None]
    return out


def _t(X):
    return np.swapaxes(X, -1, -2)


def _sym(X):
    return 0.5 * (X + _t(X))


def _dense_gradient(packed, D):
    """The symmetric dense gradient of a packed one: an off-diagonal element shared between its two positions."""
    full = rb.unpack(packed, D)
    return 0.5 * (full + full * np.eye(D, dtype=full.dtype))


def _packed_gradient(full, D):
    """The packed gradient of a symmetric dense one: an off-diagonal element counts twice."""
    doubled = 2.0 * full - full * np.eye(D, dtype=full.dtype)
    return rb.pack(doubled)


# ---- K52 / K53 ----------------------------------------------------------------------------------------------------------------------
def switching_kalman_step_backward(model, regime, state, y, grad_mean, grad_cov, grad_log_weight, observed=None,
                                   dtype=np.float64):
    """The adjoint of `testing.rao_blackwell.switching_kalman_step` (with `observed`: of `testing.switching_missing`'s) with
    the regime given and no ancestors.  model: `rb.operands`; regime int [B,K]; state: None (step 0) or (mean [B,K,D], cov
    [B,K,D(D+1)/2]); y [B,Dy]; the arriving gradients grad_mean [B,K,D], grad_cov [B,K,D(D+1)/2], grad_log_weight [B,K];
    observed: None or bool [B,Dy].  Returns (a dict of STEP_OUTPUTS — the per-slot two None at step 0, grad_m0 and grad_s0
    None at later steps — float64, flags).

    A slot whose arriving gradients are all exactly zero contributes exactly nothing and has zero rows, whatever its forward
    is; a regime outside [0, M): FLAG_INDEX_OUT_OF_RANGE, NaN rows, nothing added to any sum; a pivot that is not positive:
    NaN."""
    f = lambda x: np.asarray(x, dtype=np.float64).astype(dtype)
    regime = np.asarray(regime)
    B, K = regime.shape
    M, D, Dy = model["A"].shape[0], model["A"].shape[-1], model["C"].shape[-2]
    outside = (regime < 0) | (regime >= M)
    s = np.where(outside, 0, regime)
    mu, g = f(grad_mean), f(grad_log_weight)
    G = _dense_gradient(f(grad_cov), D)
    silent = (g == 0) & (mu == 0).all(axis=-1) & (np.asarray(grad_cov) == 0).all(axis=-1)
    A, b, q, C, d, r = (f(model[name])[s] for name in ("A", "b", "q", "C", "d", "r"))
    eye_d, eye_y = np.eye(D, dtype=dtype), np.eye(Dy, dtype=dtype)
    later = state is not None
    with np.errstate(all="ignore"):
        if later:
            m, P = f(state[0]), rb.unpack(f(state[1]), D)
            predicted = (A @ m[..., None])[..., 0] + b
            W = A @ P
            spread = W @ _t(A) + q[..., :, None] * q[..., None, :] * eye_d
        else:
            predicted = np.broadcast_to(f(model["m0"]), (B, K, D)).copy()
            spread = np.broadcast_to(f(model["s0"]) ** 2 * eye_d, (B, K, D, D)).copy()
        seen = np.ones((B, 1, Dy), dtype=bool) if observed is None else np.asarray(observed, dtype=bool)[:, None, :]
        seen = np.broadcast_to(seen, (B, K, Dy))
        C = np.where(seen[..., None], C, 0.0)
        value = np.broadcast_to(f(np.where(seen[:, 0], np.asarray(y, dtype=np.float64), 0.0))[:, None, :], (B, K, Dy))
        e = np.where(seen, value - d - (C @ predicted[..., None])[..., 0], 0.0)
        U = C @ spread
        S = U @ _t(C) + np.where(seen, r * r, 1.0)[..., :, None] * eye_y
        L = _cholesky(S)
        v = _solve_lower(L, e[..., None])
        V = _solve_lower(L, U)
        z = V @ mu[..., None]
        alpha, t = _solve_upper(L, v), _solve_upper(L, z)
        e_bar = (t - g[..., None, None] * alpha)[..., 0]
        U_bar = _solve_upper(L, v @ mu[..., None, :] - 2.0 * (V @ G))
        S_hat = 0.5 * g[..., None, None] * (v @ _t(v) - seen[..., :, None] * eye_y) - _sym(z @ _t(v)) + V @ G @ _t(V)
        S_bar = _solve_upper(L, _t(_solve_upper(L, S_hat)))
        S_bar = _sym(S_bar)
        H_hat = U_bar + S_bar @ C
        P_bar = G + _sym(_t(C) @ H_hat)
        m_bar = mu - (_t(C) @ e_bar[..., None])[..., 0]
        rows = {"grad_C": np.where(seen[..., None], (H_hat + S_bar @ C) @ spread - e_bar[..., :, None] * predicted[..., None, :], 0.0),
                "grad_d": np.where(seen, -e_bar, 0.0),
                "grad_r": np.where(seen, 2.0 * r * np.diagonal(S_bar, axis1=-2, axis2=-1), 0.0)}
        diagonal = np.diagonal(P_bar, axis1=-2, axis2=-1)
        if later:
            rows.update(grad_A=2.0 * (P_bar @ W) + m_bar[..., :, None] * m[..., None, :], grad_b=m_bar, grad_q=2.0 * q * diagonal)
            slots = {"grad_mean_in": (_t(A) @ m_bar[..., None])[..., 0], "grad_cov_in": _packed_gradient(_t(A) @ P_bar @ A, D)}
            whole = {}
        else:
            rows.update(grad_A=np.zeros((B, K, D, D), dtype=dtype), grad_b=np.zeros((B, K, D), dtype=dtype),
                        grad_q=np.zeros((B, K, D), dtype=dtype))
            slots = {}
            whole = {"grad_m0": m_bar, "grad_s0": 2.0 * f(model["s0"]) * diagonal}
    singular = ~silent & ~outside & ~np.isfinite(np.diagonal(L, axis1=-2, axis2=-1)).all(axis=-1)
    out = dict.fromkeys(STEP_OUTPUTS)
    counted = ~silent & ~outside
    lead = lambda flag, array: flag.reshape(flag.shape + (1,) * (array.ndim - 2))
    for name, array in slots.items():
        array = np.where(lead(singular, array), np.nan, array)
        array = np.where(lead(silent, array), 0.0, array)
        out[name] = np.where(lead(outside, array), np.nan, array).astype(np.float64)
    for name, array in list(rows.items()) + list(whole.items()):
        array = np.where(lead(singular, array), np.nan, np.where(lead(counted, array), array, 0.0))
        if name in whole:
            out[name] = array.sum(axis=(0, 1)).astype(np.float64)
        else:
            out[name] = np.stack([np.where(lead(regime == j, array), array, 0.0).sum(axis=(0, 1)) for j in range(M)]) \
                .astype(np.float64)
    return out, (rb.FLAG_INDEX_OUT_OF_RANGE if bool(outside.any()) else 0)


def example_step_backward(B, K, M, D, Dy, later=True, observation_dtype=np.float64, masked=False, seed=0):
    """(model, regime, state, y, grad_mean, grad_cov, grad_log_weight, observed) of one launch of K52 / K53:
    `rb.example_step`'s model, state and observation, a random regime per slot and `randn` arriving gradients for all three
    outputs, so that every slot counts.  masked: a random mask (row 0 with everything measured where B > 1, no row with
    nothing measured unless Dy == 1 forces it) and NaN at the unmeasured positions of y."""
    model, state, _, _, y = rb.example_step(B, K, M, D, Dy, later=later, observation_dtype=observation_dtype, seed=seed)
    rng = np.random.default_rng([seed, B, K, M, D, Dy, 52])
    regime = rng.integers(0, M, (B, K)).astype(np.int32)
    TD = D * (D + 1) // 2
    grads = (rng.standard_normal((B, K, D)), rng.standard_normal((B, K, TD)), rng.standard_normal((B, K)))
    observed = None
    if masked:
        observed = rng.uniform(size=(B, Dy)) < 0.6
        observed[0] = True
        for row in range(1, B):
            if not observed[row].any() and row % 2:
                observed[row, rng.integers(0, Dy)] = True
        y = np.where(observed, y, np.nan).astype(observation_dtype)
    return (model, regime, None if state is None else state[1:], y) + grads + (observed,)


# ---- K54 ------------------------------------------------------------------------------------------------------------------------------
def switching_collapse_backward(mean, cov, log_weight, grad_log_mass, grad_mean_out, grad_cov_out, dtype=np.float64):
    """The adjoint of `testing.switching_collapsed.switching_collapse`: (grad_log_weight [B,G,N], grad_mean, grad_cov in the
    layout of mean and cov — [B,G,N,.], or [B,N,.] for shared components: the sum over the row's groups), float64.  A
    component of weight -inf is not read and gets zeros; a group whose weights are all -inf gives zeros; a NaN weight gives
    NaN for its group."""
    f = lambda x: np.asarray(x, dtype=np.float64).astype(dtype)
    lw = np.asarray(log_weight, dtype=np.float64)
    B, G, N = lw.shape
    mean, cov = np.asarray(mean), np.asarray(cov)
    shared = mean.ndim == 3
    if shared:
        mean, cov = mean[:, None], cov[:, None]
    D = mean.shape[-1]
    TD = D * (D + 1) // 2
    skip = np.isneginf(lw)
    bad = np.isnan(lw).any(axis=2)
    with np.errstate(all="ignore"):
        top = np.where(bad, 0.0, lw.max(axis=2, initial=-np.inf))
        empty = ~bad & np.isneginf(top)
        top = np.where(empty, 0.0, top)
        weight = np.where(skip, 0.0, np.exp(f(lw) - f(top)[..., None]))
        weight = weight / np.where(empty | bad, 1.0, weight.sum(axis=2))[..., None]
        m = np.where(skip[..., None], 0.0, f(np.where(skip[..., None], 0.0, np.broadcast_to(mean, (B, G, N, D)))))
        P = np.where(skip[..., None], 0.0, f(np.where(skip[..., None], 0.0, np.broadcast_to(cov, (B, G, N, TD)))))
        centre = (weight[..., None] * m).sum(axis=2)
        dev = np.where(skip[..., None], 0.0, m - centre[:, :, None, :])
        a_bar, mu, c = f(grad_log_mass), f(grad_mean_out), f(grad_cov_out)
        outer = np.stack([dev[..., i] * dev[..., j] for i in range(D) for j in range(i + 1)], axis=-1)
        omega = (mu[:, :, None, :] * dev).sum(axis=-1) + (c[:, :, None, :] * (P + outer)).sum(axis=-1)
        grad_lw = weight * (a_bar[..., None] + omega - (weight * omega).sum(axis=2)[..., None])
        dense = _dense_gradient(c, D)
        grad_m = weight[..., None] * (mu[:, :, None, :] + 2.0 * np.einsum("bgps,bgns->bgnp", dense, dev))
        grad_P = weight[..., None] * c[:, :, None, :]
    out = []
    for array in (grad_lw, grad_m, grad_P):
        lead = lambda flag: flag.reshape(flag.shape + (1,) * (array.ndim - 2))
        array = np.where(lead(empty), 0.0, array)
        array = np.where(lead(bad), np.nan, array).astype(np.float64)
        out.append(array)
    if shared:
        out[1], out[2] = out[1].sum(axis=1), out[2].sum(axis=1)
    return tuple(out)


def example_collapse_backward(B, G, N, D, seed=0):
    """`randn` gradients arriving at (log_mass [B,G], mean_out [B,G,D], cov_out [B,G,D(D+1)/2]) of
    `switching_collapsed.example_collapse(B, G, N, D)`."""
    rng = np.random.default_rng([seed, B, G, N, D, 54])
    return rng.standard_normal((B, G)), rng.standard_normal((B, G, D)), rng.standard_normal((B, G, D * (D + 1) // 2))


# ---- the whole pass, restated in torch ---------------------------------------------------------------------------------------------
def safe_log(probabilities):
    """log p with -inf at p == 0 and a gradient of exactly 0 there (torch.log's backward gives 0 / 0 = NaN)."""
    positive = probabilities > 0
    return torch.where(positive, torch.log(torch.where(positive, probabilities, torch.ones_like(probabilities))),
                       torch.full_like(probabilities, -math.inf))


def expand_parameters(parameters):
    """The ten tensors in the shapes a step takes: a leading 1 expanded to M, s0 to D values (views: autograd sums)."""
    p = {name: parameters[name] for name in PARAMETERS}
    M, D, Dy = p["pi0"].numel(), p["A"].size(-1), p["C"].size(-2)
    shapes = {"A": (M, D, D), "b": (M, D), "q": (M, D), "C": (M, Dy, D), "d": (M, Dy), "r": (M, Dy)}
    out = {name: p[name].expand(shape) for name, shape in shapes.items()}
    out.update(pi0=p["pi0"], Pi=p["Pi"], m0=p["m0"], s0=p["s0"].reshape(-1).expand(D))
    return out


def _update(mean, cov, C, d, r, y, keep, excluded):
    """The Kalman update of dense (mean [..,D], cov [..,D,D]) under (C [..,Dy,D], d, r [..,Dy]) for y [..,Dy], the rows
    `keep` (a list, or None: all) of the observation alone; `excluded` [..] bool: slots whose result nothing reads — their
    innovation covariance is replaced by the identity so that a singular one there cannot reach a gradient."""
    if keep is not None:
        C, d, r, y = C[..., keep, :], d[..., keep], r[..., keep], y[..., keep]
    n = C.size(-2)
    if n == 0:
        return mean, cov, mean.new_zeros(mean.shape[:-1])
    S = C @ cov @ C.transpose(-1, -2) + torch.diag_embed(r * r)
    if excluded is not None:
        S = torch.where(excluded[..., None, None], torch.eye(n, dtype=S.dtype, device=S.device).expand_as(S), S)
    L = torch.linalg.cholesky(S)
    e = (y - d - (C @ mean.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1)
    U = C @ cov
    v = torch.linalg.solve_triangular(L, e, upper=False)
    V = torch.linalg.solve_triangular(L, U, upper=False)
    log_likelihood = -0.5 * (v * v).sum(dim=(-1, -2)) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - \
        n * rb.HALF_LOG_2PI
    return mean + (V.transpose(-1, -2) @ v).squeeze(-1), cov - V.transpose(-1, -2) @ V, log_likelihood


def _step(mean, cov, later, p, regimes, y, mask, excluded):
    """Predict (later steps) and update of slots [B,S] under `regimes` ([S], a list: the same in every batch row; or an
    integer tensor [B,S]); mask: None or bool [B,Dy]."""
    A, b, q, C, d, r = (p[name][regimes] for name in ("A", "b", "q", "C", "d", "r"))
    if A.dim() == 3:
        A, b, q, C, d, r = (x.expand((mean.size(0),) + tuple(x.shape)) for x in (A, b, q, C, d, r))
    if later:
        mean = (A @ mean.unsqueeze(-1)).squeeze(-1) + b
        cov = A @ cov @ A.transpose(-1, -2) + torch.diag_embed(q * q)
    y = y.to(torch.float64).unsqueeze(1)
    if mask is None:
        return _update(mean, cov, C, d, r, y.expand(-1, mean.size(1), -1), None, excluded)
    rows = []
    for row in range(mean.size(0)):
        keep = [i for i in range(mask.size(1)) if bool(mask[row, i])]
        rows.append(_update(mean[row], cov[row], C[row], d[row], r[row], torch.nan_to_num(y[row]).expand(mean.size(1), -1), keep,
                            None if excluded is None else excluded[row]))
    return tuple(torch.stack(part) for part in zip(*rows))


def _collapse(mean, cov, log_weight):
    """The moment-matching collapse over the last component axis: mean [..,N,D], cov [..,N,D,D], log_weight [..,N]."""
    dead = log_weight == -math.inf
    empty = dead.all(dim=-1)      # a group without a live component: mass -inf, zero moments, no gradient
    log_weight = torch.where(empty.unsqueeze(-1), torch.zeros_like(log_weight), log_weight)
    mass = torch.logsumexp(log_weight, dim=-1)
    weight = torch.where(dead, torch.zeros_like(log_weight), torch.exp(log_weight - mass.unsqueeze(-1)))
    mass = torch.where(empty, torch.full_like(mass, -math.inf), mass)
    mean = torch.where(dead[..., None], torch.zeros_like(mean), mean)
    cov = torch.where(dead[..., None, None], torch.zeros_like(cov), cov)
    centre = (weight.unsqueeze(-1) * mean).sum(dim=-2)
    dev = torch.where(dead[..., None], torch.zeros_like(mean), mean - centre.unsqueeze(-2))
    spread = (weight[..., None, None] * (cov + dev.unsqueeze(-1) * dev.unsqueeze(-2))).sum(dim=-3)
    return mass, centre, spread


def collapsed_log_likelihood_restated(observations, parameters, order=2, observed=None):
    """The collapsed-mixture log-evidence [B] of `rao_blackwell.collapsed_switching_filter`'s docstring, differentiable in the
    ten `parameters` (a mapping of float64 tensors on the observations' device, a leading 1 for shared ones), in plain
    torch.  observed: None or per timestep None or a bool [B,Dy] mask; y at an unmeasured position is not used."""
    p = expand_parameters(parameters)
    M, D = p["pi0"].numel(), p["A"].size(-1)
    B = observations[0].size(0)
    log_pi0, log_Pi = safe_log(p["pi0"]), safe_log(p["Pi"])
    every = list(range(M))
    scored = lambda prior, likelihood: torch.where(prior == -math.inf, prior, prior + likelihood)
    total = log_mu = mean = cov = None
    for time, y in enumerate(observations):
        mask = None if observed is None else observed[time]
        if time == 0:
            prior = log_pi0.expand(B, M)
            mean = p["m0"].expand(B, M, D)
            cov = torch.diag_embed(p["s0"] * p["s0"]).expand(B, M, D, D)
            mean, cov, likelihood = _step(mean, cov, False, p, every, y, mask, prior == -math.inf)
            g = scored(prior, likelihood)
        else:
            prior = log_mu.unsqueeze(1) + log_Pi.t().unsqueeze(0)      # [b,j,i]
            if order == 2:
                pairs = [j for j in range(M) for _ in range(M)]
                pair_mean, pair_cov, likelihood = _step(mean.repeat(1, M, 1), cov.repeat(1, M, 1, 1), True, p, pairs, y, mask,
                                                        (prior == -math.inf).reshape(B, M * M))
                scores = scored(prior, likelihood.reshape(B, M, M))
                g, mean, cov = _collapse(pair_mean.reshape(B, M, M, D), pair_cov.reshape(B, M, M, D, D), scores)
            else:
                mass, mixed_mean, mixed_cov = _collapse(mean.unsqueeze(1).expand(B, M, M, D),
                                                        cov.unsqueeze(1).expand(B, M, M, D, D), prior)
                mean, cov, likelihood = _step(mixed_mean, mixed_cov, True, p, every, y, mask, mass == -math.inf)
                g = scored(mass, likelihood)
        increment = torch.logsumexp(g, dim=-1)
        log_mu = g - increment.unsqueeze(-1)
        total = increment if total is None else total + increment
    return total
