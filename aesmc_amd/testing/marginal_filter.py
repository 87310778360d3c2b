"""NumPy statement of the CONTRACT of the pairwise weighted pass (include/aesmc_hip.h, aesmc_pairwise_pass, kernel K25),
written without regard to the kernel's structure (no tiles, no chunks of dimensions, no butterflies) — what the tests hold
the HIP result to — of the bound it is held to, of the backward of the pairwise log-sum-exp (K22) as two such passes, and
of the whole forward recursion that `aesmc_amd.marginal_filter` makes of K22: the marginal particle filter (Klaas, de
Freitas & Doucet 2005; as a training objective: Lai, Domke & Sheldon 2022).

`own` [B,N,D] are the points a result belongs to, `others` [B,M,D] the points summed over:

    q[n,m]        = sum_d ((own[b,n,d] - others[b,m,d]) * inv[d])^2              (inv = 1 / scale, d ascending: K22's chain)
    p[n,m]        = exp(own_term[b,n] + other_term[b,m] - q[n,m] / 2)
    w[n,m]        = p[n,m] * own_gain[b,n] * other_gain[b,m]                      (a gain of None is 1)
    mass[b,n]     = sum_m w[n,m]
    pull[b,n,d]   = sum_m w[n,m] * (others[b,m,d] - own[b,n,d]) * inv[d]^2
    spread[b,n,d] = sum_m w[n,m] * ((own[b,n,d] - others[b,m,d]) * inv[d])^2

in float64 whatever the operands' dtype is.  (This package never imports the oracle — tests/test_library.py.)
"""
import numpy as np

from .smoothing import (EPSILON, EXP_UNDERFLOW, FLAG_NAN_LOG_WEIGHT, NEAR_THE_MAXIMUM, pairwise_lse,
                        pairwise_lse_bound)

# the `c` of `pairwise_pass_bound`: what a term w * f may differ by between two evaluations beyond its exponent and the
# order of the sum, in units of eps = 2^-52 = 2 u (derived in that docstring: 13, rounded up for the second order)
TERM_ROUNDINGS = 16
TINY = 2.0 ** -1074      # the smallest positive float64: the spacing of everything below 2^-1022


def _pass_operands(own, others, scale, own_term, other_term, own_gain, other_gain):
    """float64 (own [B,N,D], others [B,M,D], inv [D], own_term [B,N], other_term [B,M], own_gain, other_gain)."""
    own_term, other_term = np.asarray(own_term), np.asarray(other_term)
    (B, N), M = own_term.shape, other_term.shape[1]
    wide = lambda a: None if a is None else np.asarray(a).astype(np.float64)
    D = 0 if own is None else int(np.prod(np.asarray(own).shape[2:], dtype=np.int64))
    inv = np.zeros(0)
    if D:
        inv = 1.0 / np.broadcast_to(wide(scale).reshape(-1), (D,))
        own, others = wide(own).reshape(B, N, D), wide(others).reshape(B, M, D)
    else:
        own, others = np.zeros((B, N, 0)), np.zeros((B, M, 0))
    ones = lambda gain, shape: np.ones(shape) if gain is None else wide(gain)
    return own, others, inv, wide(own_term), wide(other_term), ones(own_gain, (B, N)), ones(other_gain, (B, M))


def _pass_row(own, others, inv, own_term, other_term, own_gain, other_gain):
    """Everything of one batch row: (w [N,M], diff [N,M,D], q [N,M], e [N,M], present [M], live [N], nan [N])."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (own[:, None, :] - others[None, :, :]) * inv
        q = np.zeros(diff.shape[:2])
        for d in range(diff.shape[2]):
            q = q + diff[:, :, d] ** 2
        e = (own_term[:, None] + other_term[None, :]) - 0.5 * q
        present, live = other_term != -np.inf, np.isfinite(own_term)
        p = np.where(e > EXP_UNDERFLOW, np.exp(np.minimum(e, 709.0)), 0.0)
        p = np.where(np.isnan(e) | (e == np.inf), np.nan, p)
        w = np.where(present[None, :] & live[:, None], (p * own_gain[:, None]) * other_gain[None, :], 0.0)
        diff = np.where(present[None, :, None], diff, 0.0)      # an absent other is SELECTED out, never multiplied by 0
    return w, diff, q, e, present, live, np.isnan(w).any(axis=1)


def pairwise_pass(own, others, scale, own_term, other_term, own_gain=None, other_gain=None):
    """own [B,N,...], others [B,M,...] (trailing dims flattened to D values; none, or own = others = None: no distance
    term, pull and spread are [B,N,0]), scale one value or [D], own_term / own_gain [B,N], other_term / other_gain [B,M]
    -> (mass float64 [B,N], pull float64 [B,N,D], spread float64 [B,N,D], flags), as the module's docstring states them.

    Conventions, per own point (own points and batch rows never affect one another):
      an other with other_term == -inf is ABSENT: it contributes a selected zero, whatever it holds (NaN, inf);
      an own point whose own_term is not finite (-inf: an absent column; +inf or NaN: a row point whose forward value was
        -inf, +inf or NaN — the forward raised what there was to raise): zeros and no flag;
      else a NaN or +inf exponent, or a NaN weight, against a present other (a NaN other_term, coordinate, scale or
        gain): FLAG_NAN_LOG_WEIGHT and NaN in all of its outputs.
    The coordinates of a present other and of an own point with a finite own_term must be finite or NaN."""
    own, others, inv, own_term, other_term, own_gain, other_gain = _pass_operands(own, others, scale, own_term, other_term,
                                                                                  own_gain, other_gain)
    B, N, D = own.shape
    mass, pull, spread = np.empty((B, N)), np.empty((B, N, D)), np.empty((B, N, D))
    flags = 0
    for b in range(B):
        w, diff, _, _, _, live, nan = _pass_row(own[b], others[b], inv, own_term[b], other_term[b], own_gain[b],
                                                other_gain[b])
        with np.errstate(invalid="ignore", over="ignore"):
            row_mass = w.sum(axis=1)
            row_pull = (w[:, :, None] * (-diff) * inv).sum(axis=1)
            row_spread = (w[:, :, None] * diff ** 2).sum(axis=1)
        finish = lambda v, mask: np.where(nan.reshape(mask.shape), np.nan, np.where(mask, v, 0.0))
        mass[b] = finish(row_mass, live)
        pull[b], spread[b] = finish(row_pull, live[:, None]), finish(row_spread, live[:, None])
        if nan.any():
            flags |= FLAG_NAN_LOG_WEIGHT
    return mass, pull, spread, flags


def pairwise_pass_bound(own, others, scale, own_term, other_term, own_gain=None, other_gain=None):
    """(mass [B,N], pull [B,N,D], spread [B,N,D]) float64: how far a float64 evaluation of `pairwise_pass` in another order
    (other tiles, per-lane partial sums, fused against separately rounded multiply-adds, a reciprocal scale against a true
    division) may lie from this one, derived and not measured.  Every output is a sum X = sum_m t_m; with eps = 2^-52 =
    2 u (u the unit roundoff), D values per point and M others

        bound = eps * ( (D + 4) * max_m (|own_term| + |other_term[m]| + q[n,m] / 2)  +  M + c ) * sum_m |t_m|,    c = 16

    the maximum over the present others whose exponent lies within 40 of the own point's largest.  The derivation, to
    first order, for one term t = w f with w = exp(e) * own_gain * other_gain:
      * the exponent e = own_term + other_term - q / 2: q as in `pairwise_argmax_bound` ((D + 3) eps q / 2 between two
        evaluations), the two terms' sum one rounding (eps (|own_term| + |other_term|)), the last subtraction one (eps |e|):
        together at most eps (D + 4) (|own_term| + |other_term| + q / 2), and exp turns a move of the exponent into the same
        RELATIVE move of the term — the first part of the bound, taken where the terms that matter are;
      * exp itself, two implementations of two eps each: 4 eps;  the two gains, two products: 2 eps between two evaluations;
      * the factor f: for pull (others - own) * inv * inv is one subtraction, the reciprocal against a division, two
        products: 4 u per evaluation, 4 eps between two; for spread ((own - others) * inv)^2 is 3 u before the square,
        6 u after it: 6 eps between two; for mass f = 1;
      * the product w f: 1 eps between two.  Together c = 4 + 2 + 6 + 1 = 13, stated as 16 for the terms of second order;
      * the M additions, in any order: at most eps M times the sum of the magnitudes between two evaluations.
    Float64 has no relative accuracy below 2^-1022 (gradual underflow), where the tail of a sharply peaked softmax lives:
    there a weight, and its product with the factor, is a multiple of tiny = 2^-1074 and wrong by up to tiny / 2 in either
    evaluation whatever eps says, which the factor magnifies.  So the bound has the absolute floor
        2 * tiny * (M + 2) * max_m ((1 + |own_gain other_gain[m]|) * (1 + |f_m|))
    (far below anything that matters: 1e-300 at M = 1e6 and |f| = 1e15).
    Everything else is relative to sum_m |t_m|, the sum of the terms' MAGNITUDES: the bound is written for terms formed from
    differences, so an evaluation that accumulates raw moments of `others` and subtracts afterwards has to meet it all
    the same (it cannot once both clouds sit far from the origin, unless it centres them).  Zero where the own point is
    not live or is flagged (those are conventions, held exactly)."""
    own, others, inv, own_term, other_term, own_gain, other_gain = _pass_operands(own, others, scale, own_term, other_term,
                                                                                  own_gain, other_gain)
    B, N, D = own.shape
    M = others.shape[1]
    mass, pull, spread = np.zeros((B, N)), np.zeros((B, N, D)), np.zeros((B, N, D))
    for b in range(B):
        w, diff, q, e, present, live, nan = _pass_row(own[b], others[b], inv, own_term[b], other_term[b], own_gain[b],
                                                      other_gain[b])
        good = live & ~nan
        with np.errstate(invalid="ignore", over="ignore"):
            held = np.where(present[None, :] & ~np.isnan(e), e, -np.inf)
            near = held >= (held.max(axis=1) - NEAR_THE_MAXIMUM)[:, None]
            size = np.where(near & present[None, :],
                            np.abs(own_term[b])[:, None] + np.abs(other_term[b])[None, :] + 0.5 * q, 0.0).max(axis=1)
            factor = EPSILON * ((D + 4) * np.where(good, size, 0.0) + M + TERM_ROUNDINGS)
            magnitude = np.abs(np.where(good[:, None], w, 0.0))
            gains = np.where(present[None, :], 1.0 + np.abs(own_gain[b][:, None] * other_gain[b][None, :]), 0.0)
            gains = np.where(np.isfinite(gains), gains, 0.0)
            floor = 2.0 * TINY * (M + 2)
            mass[b] = factor * magnitude.sum(axis=1) + floor * gains.max(axis=1)
            pull[b] = factor[:, None] * (magnitude[:, :, None] * np.abs(diff) * inv).sum(axis=1) + \
                floor * np.nan_to_num(gains[:, :, None] * (1.0 + np.abs(diff) * inv)).max(axis=1, initial=0.0)
            spread[b] = factor[:, None] * (magnitude[:, :, None] * diff ** 2).sum(axis=1) + \
                floor * np.nan_to_num(gains[:, :, None] * (1.0 + diff ** 2)).max(axis=1, initial=0.0)
        mass[b], pull[b], spread[b] = (np.where(good.reshape((-1,) + (1,) * (v.ndim - 1)), v, 0.0)
                                       for v in (mass[b], pull[b], spread[b]))
    return mass, pull, spread


# ---- K22's backward: two passes --------------------------------------------------------------------------------------------
def _backward_terms(col_a, col_sub, row_add, out):
    """float64 (L [B,R] = out - row_add, formed from the forward's STORED result; term [B,C] = col_a - col_sub, -inf where
    col_a is -inf; -L as an other's term: -inf where L is not finite — a row point without a finite forward value is
    absent from the columns' sums, as it gets zeros in its own)."""
    wide = lambda a: None if a is None else np.asarray(a).astype(np.float64)
    col_a, col_sub, row_add, out = wide(col_a), wide(col_sub), wide(row_add), wide(out)
    with np.errstate(invalid="ignore"):
        L = out if row_add is None else out - row_add
        term = col_a if col_sub is None else np.where(col_a == -np.inf, -np.inf, col_a - col_sub)
    return L, term, np.where(np.isfinite(L), -L, -np.inf)


def pairwise_lse_backward(rows, cols, scale, col_a, col_sub, row_add, out, grad_out):
    """The gradients of `pairwise_lse`'s six operands for the gradient `grad_out` [B,R] arriving at its result `out`
    [B,R] (the forward's stored value, not recomputed), in float64 whatever the operands' dtype is, as two `pairwise_pass`
    calls.  With L = out - row_add and term = col_a - col_sub:

        rows side   own = rows, others = cols, own_term = -L, other_term = term, own_gain = grad_out:
                    grad_rows = pull,  grad_scale[d] = sum_{b,r} spread[b,r,d] / scale[d]  (summed over d too for a scale of
                    one value),  mass = grad_out (a check: returned as "mass")
        cols side   own = cols, others = rows, own_term = term, other_term = -L, other_gain = grad_out:
                    grad_col_a = mass,  grad_col_sub = -mass,  grad_cols = pull
        grad_row_add = grad_out

    Returns (dict with keys rows, cols, scale, col_a, col_sub, row_add, mass; flags).  A D == 0 launch has no rows, cols
    or scale gradient (empty arrays)."""
    L, term, absent_or_minus_l = _backward_terms(col_a, col_sub, row_add, out)
    g = np.asarray(grad_out).astype(np.float64)
    mass_rows, pull_rows, spread_rows, flags_rows = pairwise_pass(rows, cols, scale, -L, term, own_gain=g)
    mass_cols, pull_cols, _, flags_cols = pairwise_pass(cols, rows, scale, term, absent_or_minus_l, other_gain=g)
    grad_scale = np.zeros(0)
    if spread_rows.shape[2]:
        wide_scale = np.asarray(scale).astype(np.float64).reshape(-1)
        grad_scale = spread_rows.sum(axis=(0, 1)) / np.broadcast_to(wide_scale, (spread_rows.shape[2],))
        if wide_scale.size == 1:
            grad_scale = grad_scale.sum(keepdims=True)
    grads = dict(rows=pull_rows, cols=pull_cols, scale=grad_scale, col_a=mass_cols, col_sub=-mass_cols, row_add=g,
                 mass=mass_rows)
    return grads, flags_rows | flags_cols


def pairwise_lse_backward_bound(rows, cols, scale, col_a, col_sub, row_add, out, grad_out):
    """`pairwise_pass_bound` of the two passes, under `pairwise_lse_backward`'s keys; the scale's adds eps (B R + D + 2)
    times the magnitudes for the caller's own reduction and division."""
    L, term, absent_or_minus_l = _backward_terms(col_a, col_sub, row_add, out)
    g = np.asarray(grad_out).astype(np.float64)
    mass_rows, pull_rows, spread_rows = pairwise_pass_bound(rows, cols, scale, -L, term, own_gain=g)
    mass_cols, pull_cols, _ = pairwise_pass_bound(cols, rows, scale, term, absent_or_minus_l, other_gain=g)
    bound_scale = np.zeros(0)
    if spread_rows.shape[2]:
        B, R, D = spread_rows.shape
        wide_scale = np.abs(np.asarray(scale).astype(np.float64).reshape(-1))
        _, _, spread, _ = pairwise_pass(rows, cols, scale, -L, term, own_gain=np.abs(g))
        with np.errstate(invalid="ignore"):
            total = np.nan_to_num(spread).sum(axis=(0, 1))
        bound_scale = (spread_rows.sum(axis=(0, 1)) + EPSILON * (B * R + D + 2) * total) / np.broadcast_to(wide_scale, (D,))
        if wide_scale.size == 1:
            bound_scale = bound_scale.sum(keepdims=True)
    return dict(rows=pull_rows, cols=pull_cols, scale=bound_scale, col_a=mass_cols, col_sub=mass_cols,
                row_add=np.zeros(g.shape), mass=mass_rows)


# ---- the marginal particle filter ------------------------------------------------------------------------------------------
def marginal_filter_pass(latents, ancestral_indices, proposal_locations, transition_locations, proposal_scale,
                         transition_scale, emission_log_probs, first_log_weight, return_tolerance=False):
    """The whole forward recursion of the marginal particle filter over what one run stored: latents T x [B,K,...] (the
    particles as drawn), ancestral_indices T-1 x [B,K] (which ancestor each draw was proposed from — the marginal filter's
    weights do NOT depend on them, that is its point; they are checked for their shape only), proposal_locations(t) /
    transition_locations(t) -> the proposal's / transition's location [B,K,...] of step t-1's stored particles for time
    t (t = 1 .. T-1), the two scales (one value or one per latent dimension), emission_log_probs T x [B,K] = log g(y_t |
    x[t]) and first_log_weight [B,K], step 0's ordinary log-weight.  Returns (log_weights T x [B,K], log_z [B]) in
    first_log_weight's dtype:

        lf[k]      = log sum_i exp(log_v[t-1][i] - 1/2 |x[t][k] - loc_f[i]|^2)       (pairwise_lse, in units of scale_f)
        lq[k]      = log sum_i exp(log_v[t-1][i] - 1/2 |x[t][k] - loc_q[i]|^2)       (pairwise_lse, in units of scale_q)
        log_v[t]   = log g(y_t | x[t]) + ( (lf - sum_d log scale_f[d]) - (lq - sum_d log scale_q[d]) )
        log_z      = sum_t ( logsumexp_k log_v[t] - log K )

    every pairwise_lse rounded to that dtype as the device's launches round theirs, and the few operations around them in
    the dtype's own arithmetic.  With identical proposal and transition operands lf == lq and the bracket is exactly 0.
    `return_tolerance`: also (T x [B,K], [B]) float64, how far an evaluation that keeps every launch within
    `pairwise_lse_bound` (and, in float32, within one unit in the last place of the rounding) may lie from this one: a
    log-sum-exp moves by at most the largest move of its terms, so a step's tolerance is twice the largest of the step
    before it (once per launch), the two launches' bounds and last places, and four units in the last place of every
    operand of the operations around them; log_z's is the sum over the steps of the largest of each plus four units
    in the last place of the step's log-sum-exp and of the running total."""
    T = len(latents)
    first = np.asarray(first_log_weight)
    dtype = first.dtype
    B, K = first.shape
    if len(ancestral_indices) != T - 1 or any(tuple(np.asarray(i).shape) != (B, K) for i in ancestral_indices):
        raise ValueError("one [{}, {}] block of ancestor indices per resampling step ({})".format(B, K, T - 1))
    unit = float(np.finfo(dtype).eps)

    def last_place(v):      # of the rounding to the dtype: float64 results are not rounded again
        if dtype == np.float64:
            return np.zeros(v.shape)
        return np.where(np.isfinite(v), np.spacing(np.abs(np.where(np.isfinite(v), v, 0)).astype(dtype)), 0).astype(np.float64)

    def row_lse(v):
        v = v.astype(np.float64)
        top = v.max(axis=1)
        return top + np.log(np.exp(v - top[:, None]).sum(axis=1))

    def log_scales(scale, D):      # sum_d log scale[d], in the dtype
        scale = np.asarray(scale).astype(dtype).reshape(-1)
        return dtype.type(np.log(scale).sum(dtype=dtype) * dtype.type(D // scale.size))

    log_weights, tolerance = [first], [4.0 * unit * np.abs(first.astype(np.float64))]
    log_z = row_lse(first) - np.log(K)
    z_tolerance = tolerance[0].max(axis=1) + 4.0 * unit * np.abs(log_z)
    for t in range(1, T):
        x, previous = np.asarray(latents[t]), log_weights[-1]
        D = int(np.prod(x.shape[2:], dtype=np.int64))
        loc_f, loc_q = np.asarray(transition_locations(t)), np.asarray(proposal_locations(t))
        lf = pairwise_lse(x, loc_f, transition_scale, previous)[0].astype(dtype)
        lq = pairwise_lse(x, loc_q, proposal_scale, previous)[0].astype(dtype)
        cf, cq = log_scales(transition_scale, D), log_scales(proposal_scale, D)
        log_g = np.asarray(emission_log_probs[t]).astype(dtype)
        log_v = log_g + ((lf - cf) - (lq - cq))
        log_weights.append(log_v)
        wide = lambda v: np.abs(np.asarray(v, dtype=np.float64))
        tolerance.append(2.0 * tolerance[-1].max(axis=1, keepdims=True) +
                         pairwise_lse_bound(x, loc_f, transition_scale, previous) + last_place(lf) +
                         pairwise_lse_bound(x, loc_q, proposal_scale, previous) + last_place(lq) +
                         4.0 * unit * (wide(lf) + wide(lq) + wide(cf) + wide(cq) + wide(log_g) + wide(log_v)))
        step = row_lse(log_v) - np.log(K)
        log_z = log_z + step
        z_tolerance = z_tolerance + tolerance[-1].max(axis=1) + 4.0 * unit * (np.abs(step) + np.log(K) + np.abs(log_z))
    log_z = log_z.astype(dtype)
    return (log_weights, log_z, (tolerance, z_tolerance)) if return_tolerance else (log_weights, log_z)
