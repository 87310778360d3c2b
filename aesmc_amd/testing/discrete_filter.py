"""NumPy statement of the CONTRACT of the discrete particle filter (Fearnhead & Clifford 2003) for switching linear-Gaussian
state-space models: the look-ahead's scores (include/aesmc_hip.h: aesmc_switching_lookahead_scores, K43), optimal
resampling over all successor regimes (aesmc_switching_optimal_resample, K44) and the whole filter that
`aesmc_amd.rao_blackwell.discrete_switching_filter` makes of them and K31's forced step.  Written without regard to the
kernels' structure; `_lookahead`, `_step` and `_forced` are `testing.rao_blackwell`'s, by import.

Every particle proposes all M successor regimes with their exact weights; candidate i = k M + j has

    a_i = log_w[b,k] + scores[b,k,j]  (one rounded addition);   top = max_i a_i
    e_i = exp(a_i - top), 0 where a_i - top < log(2^-1022);     live: e_i > 0;     E = sum_i e_i;     lse = top + log E

(a result below the normal range is flushed: whether a candidate lives must not hang on how an exponential rounds a
subnormal).  With at most K_out live candidates all of them survive, in ascending i, with log-weight a_i - lse; the other
slots are dead (log-weight -inf, slot 0's parent and regime).  Otherwise, with w_i = e_i / E,

    c       solves sum_i min(1, w_i / c) = K_out: with the candidates by descending weight, L is the smallest number with
            e_(L+1) (K_out - L) < S_L, S_L the sum of e over all but the L heaviest; capped at K_out - 1 (equal weights
            are then kept in ascending i); c E = S_L / (K_out - L)
    kept    the L heaviest in ascending i, log-weight a_i - lse
    thinned R = K_out - L; Q_i the inclusive running sum of e over the candidates not kept, t_i = R (Q_i / Q_last): slot
            L + n takes the first live candidate not kept with t_i > n + u; log-weight (top + log(Q_last / R)) - lse

The sums may be added in any order: two evaluations can differ only where a w_i lies within rounding of c, or an n + u
within rounding of a t_i — the two margins `optimal_resample` returns, as `testing.rao_blackwell._step_margins` does for
K37.  (This package never imports the oracle — tests/test_library.py.)
"""
import numpy as np

from . import rao_blackwell as rb

UNIT = rb.UNIT
FLAG_NAN_LOG_WEIGHT, FLAG_DEGENERATE_ROW = rb.FLAG_NAN_LOG_WEIGHT, rb.FLAG_DEGENERATE_ROW
LOG_MIN_NORMAL = -708.3964185322641      # log(2^-1022)
MAX_CANDIDATES = 16384                   # aesmc_switching_optimal_resample_max_candidates()


# ---- K43: the look-ahead's scores ---------------------------------------------------------------------------------------------
def _scores(model, log_prior, state, y, num_particles, dtype, track):
    """g_j of `testing.rao_blackwell`'s look-ahead, as that function forms them: (values [B,K,M], errors or None, flags)."""
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
    flags, values, errors = 0, [], []
    for j in range(M):
        shim, forced = rb._forced(model, np.full((B, K), j))
        (_, _, _, ell, bits), (_, _, ell_e) = rb._step(shim, state, None, forced, y, dtype, track)
        flags |= bits
        excluded = np.isneginf(prior[:, :, j])
        value, error = rb._chain(given(np.where(excluded, 0.0, prior[:, :, j])), [((ell, ell_e), one)])
        values.append(np.where(excluded & ~bad, -np.inf, value))
        errors.append(np.where(excluded | np.isnan(value), 0.0, error) if track else None)
    return np.stack(values, axis=-1), (np.stack(errors, axis=-1).astype(np.float64) if track else None), flags


def _observations(y, observed):
    """(the observation as `testing.rao_blackwell` takes it, the context its primitives run in): under a mask the marked
    observation and `testing.switching_missing`'s grouped primitives — row by row the reduced model."""
    import contextlib
    if observed is None:
        return y, contextlib.nullcontext()
    from . import switching_missing as sm
    return sm.mark(y, observed), sm._masked()


def switching_lookahead_scores(model, log_prior, state, y, num_particles=None, dtype=np.float64, observed=None):
    """(scores [B,K,M], log_weight [B,K], flags) of K43: scores[b,k,j] = g_j exactly as `testing.rao_blackwell`'s look-ahead
    defines it (-inf where the log-prior is -inf, NaN where it is finite and a pivot is not positive, NaN for every j where
    the stored regime is outside [0, M) — FLAG_INDEX_OUT_OF_RANGE), and that function's log_weight.  Arguments as
    `testing.rao_blackwell.switching_lookahead`'s; observed: None or bool [B,Dy] (the masked form: K40's body)."""
    y, context = _observations(y, observed)
    with context, np.errstate(all="ignore"):
        values, _, flags = _scores(model, log_prior, state, y, num_particles, dtype, False)
        (log_weight, _, bits), _ = rb._lookahead(model, log_prior, state, y, num_particles, dtype, False)
    return values, log_weight, flags | bits


def switching_lookahead_scores_bound(model, log_prior, state, y, num_particles=None, observed=None):
    """(bound of scores [B,K,M], of log_weight [B,K]): `switching_kalman_step_bound`'s running analysis carried through the
    one addition that makes a score, 2 * 1.01 times the running bound as there; the log-weight's is
    `switching_lookahead_bound`'s.  Zero where the output is -inf or NaN."""
    y, context = _observations(y, observed)
    with context, np.errstate(all="ignore"):
        _, errors, _ = _scores(model, log_prior, state, y, num_particles, np.float64, True)
        _, (lw_e, _) = rb._lookahead(model, log_prior, state, y, num_particles, np.float64, True)
    clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
    return clean(errors), clean(lw_e)


# ---- K44: optimal resampling ----------------------------------------------------------------------------------------------------
def optimal_resample(log_w, scores, u, num_slots):
    """(parent int64 [B,K_out], regime int32 [B,K_out], log_weight [B,K_out], lse [B], count int32 [B], flags,
    margin_weight [B], margin_position [B], bound [B]) of one optimal resampling step (K44; the module's docstring).

    log_w: float64 [B,K_in] or None (zeros); scores: float64 [B,K_in,M]; u: float64 [B] in [0, 1); num_slots: K_out.
    A NaN candidate — FLAG_NAN_LOG_WEIGHT —, a maximum that is not finite — FLAG_DEGENERATE_ROW: every parent of the row
    K_in, every regime 0, log_weight and lse NaN, count 0.

    margin_weight: how far the decision "kept or thinned" is from flipping, relative to c: the smallest of (e_(L) - c) / c
    and (c - e_(L+1)) / c (the second not at L = K_out - 1, where either outcome of the test keeps the same candidates);
    where the test fails for every L (the cap) how far each failure is from passing — (e_(L+1) (K_out - L) - S_L) / S_L
    above the weight at the cut, and among the m equal weights at the cut, where m t stands against m t + tail, 1 - tail /
    (half a unit in the last place of m t): the tail behind them must not register; and the distance of every a_i - top
    from the flushing point log(2^-1022).  margin_position: the smallest
    |n + u - t_i| over the slots and the two candidates around each position, relative to 1.  inf where nothing is decided.
    bound: how far log_weight and lse of another float64 evaluation (any summation order, library exp and log within two
    units in the last place) may lie from these, derived and not measured, 2 * 1.01 times one evaluation's:

        E, Q_last   (N + 2) u + sum_i e_i (|a_i - top| + 3) u / total            (N = K_in M terms, a rounded difference, an exp)
        lse         that of E + 2 u |log E| + u + u |lse|
        kept        lse's + u |a_i - lse|;     thinned   Q_last's + u + 2 u |log(Q_last / R)| + u + u |top + log| + lse's + u |.|"""
    scores = np.asarray(scores, dtype=np.float64)
    B, K_in, M = scores.shape
    K_out, N = int(num_slots), K_in * M
    u = np.asarray(u, dtype=np.float64).reshape(B)
    parent = np.zeros((B, K_out), dtype=np.int64)
    regime = np.zeros((B, K_out), dtype=np.int32)
    log_weight = np.full((B, K_out), np.nan)
    lse, count = np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    margin_w, margin_p, bound = np.full(B, np.inf), np.full(B, np.inf), np.zeros(B)
    flags = 0
    for b in range(B):
        with np.errstate(all="ignore"):
            a = (scores[b] if log_w is None else np.asarray(log_w, dtype=np.float64)[b][:, None] + scores[b]).reshape(N)
            top = a.max() if not np.isnan(a).any() else np.nan
        if np.isnan(top) or not np.isfinite(top):
            flags |= FLAG_NAN_LOG_WEIGHT if np.isnan(top) else FLAG_DEGENERATE_ROW
            parent[b] = K_in
            continue
        with np.errstate(all="ignore"):
            x = a - top
            e = np.where(x >= LOG_MIN_NORMAL, np.exp(x), 0.0)
        live = e > 0
        finite = np.isfinite(x)
        margin_w[b] = float(np.abs(x[finite] - LOG_MIN_NORMAL).min())
        E = float(e.sum())
        lse[b] = top + np.log(E)
        size = np.where(live, e * (np.abs(np.where(finite, x, 0.0)) + 3.0), 0.0)
        lse_e = 1.01 * ((N + 2) * UNIT + UNIT * float(size.sum()) / E) + 2 * UNIT * abs(np.log(E)) + UNIT + UNIT * abs(lse[b])
        n_live = int(live.sum())
        if n_live <= K_out:
            survivors = np.flatnonzero(live)
            parent[b, :n_live], regime[b, :n_live] = survivors // M, survivors % M
            log_weight[b, :n_live] = a[survivors] - lse[b]
            parent[b, n_live:], regime[b, n_live:], log_weight[b, n_live:] = parent[b, 0], regime[b, 0], -np.inf
            count[b] = n_live
            bound[b] = 2 * 1.01 * (lse_e + UNIT * float(np.abs(log_weight[b, :n_live]).max()))
            continue
        order = np.argsort(-e, kind="stable")      # descending weight, equal weights in ascending i
        heavy = e[order]
        rest = np.cumsum(heavy[::-1])[::-1]        # rest[L] = the sum over all but the L heaviest
        tried = np.arange(K_out)
        passes = heavy[tried] * (K_out - tried) < rest[tried]
        L = int(np.argmax(passes)) if passes.any() else K_out - 1
        kept = np.zeros(N, dtype=bool)
        kept[order[:L]] = True
        R = K_out - L
        Q = np.cumsum(np.where(kept, 0.0, e))
        c = Q[-1] / R
        if passes.any():
            if L > 0:
                margin_w[b] = min(margin_w[b], float((heavy[L - 1] - c) / c))
            if L < K_out - 1:
                margin_w[b] = min(margin_w[b], float((c - heavy[L]) / c))
        else:      # the cap: the test fails for every L, and the margin is how far each failure is from passing
            cut = heavy[K_out - 1]
            tied = heavy[tried] == cut      # (they end at K_out - 1: one more equal weight behind and the test would pass)
            above = tried[~tied]
            if above.size:
                margin_w[b] = min(margin_w[b], float(((heavy[above] * (K_out - above) - rest[above]) / rest[above]).min()))
            # among the equal weights m t stands against m t + tail: it passes once the tail registers next to m t
            tail = float(rest[K_out]) if K_out < N else 0.0
            margin_w[b] = min(margin_w[b], float((1.0 - tail / (0.5 * np.spacing(cut * (K_out - tried[tied])))).min()))
        survivors = np.flatnonzero(kept)
        parent[b, :L], regime[b, :L] = survivors // M, survivors % M
        log_weight[b, :L] = a[survivors] - lse[b]
        thinned = np.flatnonzero(live & ~kept)
        t = R * (Q[thinned] / Q[-1])
        position = np.arange(R) + u[b]
        found = np.searchsorted(t, position, side="right")      # the first t_i > n + u
        around = np.stack([np.abs(t[np.minimum(found, t.size - 1)] - position),
                           np.where(found > 0, np.abs(t[np.maximum(found - 1, 0)] - position), np.inf)])
        margin_p[b] = float(around.min())
        taken = thinned[np.minimum(found, t.size - 1)]
        parent[b, L:], regime[b, L:] = taken // M, taken % M
        inner = np.log(Q[-1] / R)
        log_weight[b, L:] = (top + inner) - lse[b]
        count[b] = K_out
        q_e = 1.01 * ((N + 2) * UNIT + UNIT * float(size[thinned].sum()) / Q[-1])
        thin_e = q_e + UNIT + 2 * UNIT * abs(inner) + UNIT + UNIT * abs(top + inner) + lse_e + UNIT * abs(log_weight[b, L])
        kept_e = lse_e + UNIT * (float(np.abs(log_weight[b, :L]).max()) if L else 0.0)
        bound[b] = 2 * 1.01 * max(thin_e, kept_e)
    return parent, regime, log_weight, lse, count, flags, margin_w, margin_p, bound


# ---- the filter -----------------------------------------------------------------------------------------------------------------
def discrete_switching_pass(observations, model, num_particles, uniforms, observed=None):
    """The whole discrete particle filter on replayed uniforms (`aesmc_amd.rao_blackwell.discrete_switching_filter`): per step
    the scores on the stored system (step 0: on the prior, K_in = 1), optimal resampling with the stored log-weights, and
    `testing.rao_blackwell`'s step forced to the chosen regimes through the parents.  observations: T x [B,Dy]; model:
    `operands`' dict; uniforms: T x float64 [B]; observed: None, or T entries of None or bool [B,Dy].

    Returns a dict: log_marginal_likelihood [B] (the sum of the steps' lse); regimes, means, covariances, log_weights (T
    stored systems; the log-weights normalised, -inf in dead slots); ancestral_indices ((T-1) x int64 [B,K]); num_live (T x
    int32 [B]); flags; margins {"weights": T x [B], "positions": T x [B]} (`optimal_resample`'s); and tolerances, propagated as
    `adapted_switching_pass` propagates its own, with the factors of `_sensitivities`:

        tol_P[t], tol_m[t]   as there, from the forced step's bound
        tol_g[t]  = 1.01 max_j (wm_j tol_m[t-1] + wp_j tol_P[t-1])      (what the input state's error does to a score)
        tol_a[t]  = tol_lw[t-1] + tol_g[t] + max score bound            (a candidate: a log-weight plus a score)
        tol_lw[t] = 2 tol_a[t] + max bound of the resampling             (`log_weights`: a candidate less the log-sum-exp,
                                                                         each of which moves by at most tol_a)
        tol_Z    += tol_a[t] + max bound of the resampling."""
    T, K = len(observations), int(num_particles)
    M = model["A"].shape[0]
    if observed is None:
        observed = [None] * T
    with np.errstate(divide="ignore"):
        log_pi0, log_Pi = np.log(model["pi0"]), np.log(model["Pi"])
    out = {name: [] for name in ("regimes", "means", "covariances", "log_weights", "ancestral_indices", "num_live")}
    margins = {"weights": [], "positions": []}
    tolerances = {name: [] for name in ("means", "covariances", "scores", "log_weights")}
    state, log_w, flags = None, None, 0
    log_z, tol_z = 0.0, 0.0
    for t in range(T):
        y, context = _observations(np.asarray(observations[t]), observed[t])
        prior = log_pi0 if t == 0 else log_Pi
        K_in = 1 if t == 0 else K
        with context, np.errstate(all="ignore"):
            scores, errors, bits = _scores(model, prior, state, y, K_in, np.float64, True)
            flags |= bits
            carried = 0.0
            if t > 0:
                before_m, before_p = tolerances["means"][-1], tolerances["covariances"][-1]
                rows = log_Pi[np.clip(state[0], 0, M - 1)]
                for j in range(M):      # (a particle for which regime j is excluded stands in with its likeliest successor)
                    considered = np.where(np.isneginf(rows[:, :, j]), np.argmax(rows, axis=-1), j)
                    _, _, _, wm, wp = rb._sensitivities(model, state, None, considered, y)
                    carried = max(carried, 1.01 * (wm * before_m + wp * before_p))
            fresh = np.where(np.isfinite(errors), 2 * 1.01 * errors, 0.0)
            tol_a = (tolerances["log_weights"][-1] if t > 0 else 0.0) + carried + float(fresh.max())
            parent, chosen, log_w, lse, count, bits, margin_w, margin_p, bound = optimal_resample(log_w, scores, uniforms[t], K)
            flags |= bits
            margins["weights"].append(margin_w), margins["positions"].append(margin_p)
            log_z = log_z + lse
            tol_z += tol_a + float(bound.max())
            tolerances["scores"].append(tol_a)
            tolerances["log_weights"].append(2 * tol_a + float(bound.max()))
            idx = None if t == 0 else np.minimum(parent, K_in - 1)      # (a bad row's marker is K_in: the flag says so)
            shim, forced = rb._forced(model, chosen)
            (regime, mean, cov, _, bits), (mean_e, cov_e, _) = rb._step(shim, state, idx, forced, y, np.float64, True)
            flags |= bits
            clean = lambda e: np.where(np.isfinite(e), 2 * 1.01 * e, np.inf)
            D = mean.shape[-1]
            fresh_m = float(np.sqrt((clean(mean_e) ** 2).sum(axis=-1)).max())
            fresh_p = float(np.sqrt((rb.unpack(clean(cov_e), D) ** 2).sum(axis=(-2, -1))).max())
            if t == 0:
                tol_m, tol_p = fresh_m, fresh_p
            else:
                pp, mm, mp, _, _ = rb._sensitivities(model, state, idx, regime, y)
                tol_p = 1.01 * pp * before_p + fresh_p
                tol_m = 1.01 * (mm * before_m + mp * before_p) + fresh_m
        state = (regime, mean, cov)
        tolerances["means"].append(tol_m), tolerances["covariances"].append(tol_p)
        out["regimes"].append(regime), out["means"].append(mean), out["covariances"].append(cov)
        out["log_weights"].append(log_w), out["num_live"].append(count)
        if t > 0:
            out["ancestral_indices"].append(parent)
    tolerances["log_marginal_likelihood"] = float(tol_z)
    out.update(log_marginal_likelihood=log_z, flags=flags, tolerances=tolerances, margins=margins)
    return out


# ---- the inputs the tests share -------------------------------------------------------------------------------------------------
# (B, K_in, M, K_out): step 0 with dead slots; a few candidates; a partial wavefront; two rounds of 1024 lanes; the largest M;
# the cap of 16384 candidates; three rounds of 256 lanes
RESAMPLE_SHAPES = [(1, 1, 2, 4), (3, 7, 2, 7), (2, 65, 3, 65), (2, 300, 4, 300), (2, 5, 16, 5), (1, 1024, 16, 1024),
                   (2, 150, 4, 150)]
RESAMPLE_PROFILES = ("normal", "equal", "geometric", "dominant", "exact", "one_over", "one_parent", "cap", "cap_ties")
CAP_TIES = 5      # the equal weights of "cap_ties" (fewer where K_out is smaller)


def example_resample(B, K_in, M, K_out, profile, seed=0):
    """(log_w [B,K_in], scores [B,K_in,M], u [B]) of one optimal resampling step:

        normal      3 N(0,1) candidates, a tenth of them at -inf            equal       every candidate the same
        geometric   weights 0.93^i in a shuffled order: many are kept       dominant    one candidate holds all but 1e-12
        exact       exactly K_out live candidates                           one_over    K_out + 1 live candidates
        one_parent  every parent but one at -inf                            cap         K_out - 1 heavy candidates, one at
                                                                                        e^-10 and the rest at e^-60, whose sum
                                                                                        does not register next to it: L is capped
        cap_ties    K_out - 5 heavy candidates, FIVE bit-equal ones at e^-10 spread from the first candidate to the last (other
                    wavefronts, other rounds) and the rest at e^-70: the equal weights straddle slot K_out - 1, the test fails
                    for every L, and the cap keeps the first four of them in ascending i

    log_w is a multiple of 1/4 in [-2, 2] and the scores are the candidates less it, so that a_i has the profile to rounding."""
    rng = np.random.default_rng([seed, B, K_in, M, K_out, RESAMPLE_PROFILES.index(profile)])
    N = K_in * M
    log_w = rng.integers(-8, 9, (B, K_in)) / 4.0      # (quarters: equal candidates stay equal through the addition)
    a = np.empty((B, N))
    for b in range(B):
        if profile == "normal":
            row = 3.0 * rng.standard_normal(N)
            row[rng.permutation(N)[:N // 10]] = -np.inf
        elif profile == "equal":
            row = np.full(N, 0.25)
        elif profile == "geometric":      # (0.93: with 0.9 the L-th heaviest weight IS c, 0.9^(L-1) = 0.9^L (10 / 9))
            row = np.log(0.93) * rng.permutation(N).astype(np.float64)
        elif profile == "dominant":
            row = np.full(N, np.log(1e-12 / max(N - 1, 1))) + 0.01 * rng.standard_normal(N)
            row[rng.integers(N)] = 0.0
        elif profile in ("exact", "one_over"):
            alive = min(N, K_out + (profile == "one_over"))
            row = np.full(N, -np.inf)
            row[rng.permutation(N)[:alive]] = 2.0 * rng.standard_normal(alive)
        elif profile == "one_parent":
            row = np.full((K_in, M), -np.inf)
            row[rng.integers(K_in)] = rng.standard_normal(M)
            row = row.reshape(N)
        elif profile == "cap_ties":
            row = np.full(N, -70.0) + 0.01 * rng.standard_normal(N)
            if N > K_out:
                ties = np.unique(np.linspace(0, N - 1, min(CAP_TIES, K_out)).round().astype(np.int64))
                others = np.setdiff1d(np.arange(N), ties)
                row[rng.permutation(others)[:K_out - ties.size]] = 0.1 * rng.standard_normal(K_out - ties.size)
                row[ties] = -10.0
        else:
            row = np.full(N, -60.0) + 0.01 * rng.standard_normal(N)
            spots = rng.permutation(N)[:min(K_out, N)]
            row[spots[1:]] = 0.1 * rng.standard_normal(spots.size - 1)
            row[spots[0]] = -10.0
        a[b] = row
    if profile == "one_parent":      # (the parents themselves carry the -inf)
        alive = np.isfinite(a.reshape(B, K_in, M)).any(axis=2)
        log_w = np.where(alive, log_w, -np.inf)
        scores = np.where(alive[:, :, None], a.reshape(B, K_in, M) - np.where(alive, log_w, 0.0)[:, :, None],
                          rng.standard_normal((B, K_in, M)))
    else:
        scores = a.reshape(B, K_in, M) - log_w[:, :, None]
    return log_w, scores, rng.uniform(size=B)


def example_sweep(K_in=65, M=3, K_out=4):
    """(log_w, scores, u) of K_in M rows: row i has ONE heavy candidate, at position i, and equal light ones — the heavy one
    is kept and must come out at slot 0 with its own parent and regime."""
    N = K_in * M
    a = np.full((N, N), -3.0)
    a[np.arange(N), np.arange(N)] = 4.0
    log_w = np.tile(np.arange(K_in) % 5 / 4.0, (N, 1))
    rng = np.random.default_rng([N, K_out])
    return log_w, a.reshape(N, K_in, M) - log_w[:, :, None], rng.uniform(size=N)


# (B, K, M, D, Dy, T) of the replayed filters; (M, D, Dy, T, K) where M^T <= K: nothing is discarded and the evidence is exact
FILTER_SHAPES = [(2, 8, 2, 2, 1, 6), (2, 65, 3, 8, 8, 4)]
EXACT_SHAPES = [(2, 2, 1, 4, 16), (3, 2, 2, 3, 27), (2, 3, 2, 5, 40)]


def example_series(B, M, D, Dy, T, seed=0):
    """(model, observations: T x [B,Dy], uniforms: T x [B]) of a replayed filter: `example_model` and a series simulated from
    it per batch row (a fixed generator)."""
    model = rb.example_model(M, D, Dy, seed)
    rng = np.random.default_rng([seed, B, M, D, Dy, T])
    observations, s, z = [], None, None
    for t in range(T):
        if t == 0:
            s = np.array([rng.choice(M, p=model["pi0"]) for _ in range(B)])
            z = model["m0"] + model["s0"] * rng.standard_normal((B, D))
        else:
            s = np.array([rng.choice(M, p=model["Pi"][before]) for before in s])
            z = np.einsum("bij,bj->bi", model["A"][s], z) + model["b"][s] + model["q"][s] * rng.standard_normal((B, D))
        observations.append(np.einsum("bij,bj->bi", model["C"][s], z) + model["d"][s] +
                            model["r"][s] * rng.standard_normal((B, Dy)))
    return model, observations, [rng.uniform(size=B) for _ in range(T)]
