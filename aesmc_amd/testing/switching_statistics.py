"""The NumPy (float64) contract of the switching-model EM statistics: kernels K45 / K46
(`aesmc_switching_moment_statistics`, `aesmc_switching_masked_moment_statistics`, with `aesmc_switching_statistics_finish`),
and of `rao_blackwell.switching_expected_statistics`, `switching_m_step` and `switching_score` on top of them.

Along a regime trajectory (b, n) the model is linear-Gaussian, and K36 gives the smoothed N(m_t, P_t) of z_t with the lag-one
cross_{t-1}[i,l] = Cov(z_{t,i}, z_{t-1,l}) (rows at the later time).  With x = (z, 1) in R^X, X = D + 1,

    E[x_t x_t^T] = [[P_t + m_t m_t^T, m_t], [m_t^T, 1]]        E[z_t x_{t-1}^T] = [cross_{t-1} + m_t m_{t-1}^T, m_t]

and with j = s_t, i = s_{t-1}, o_c whether component c of y_t[b] was observed (no mask: 1), one timestep adds to ROW j

    transition_counts (stored [i, j])   1[s_{t-1} = i]                t >= 1
    next_next   [D, D]                  E[z_t z_t^T]                  t >= 1
    next_prev   [D, X]                  E[z_t x_{t-1}^T]              t >= 1
    prev_prev   [X, X]                  E[x_{t-1} x_{t-1}^T]          t >= 1
    obs_obs     [Dy]                    o_c y_c^2                     t >= 0
    obs_state   [Dy, X]                 o_c y_c E[x_t]^T              t >= 0
    state_state [Dy, X, X]              o_c E[x_t x_t^T]              t >= 0

summed over all (b, n).  The t = 0 step goes into a block of its own: `initial_counts[j]` is the "1 1" entry of row j of its
unmasked gram, `initial_state` [X, X] the sum of that gram over j (it gives m0 and s0); the emission totals are the t = 0 block
plus the later one.

The kernel's layout is one [16, F] array per block (`layout`): row = regime, the symmetric matrices as packed lower triangles
(element (i, l), i >= l, at i (i + 1) / 2 + l; the constant's index is D), in the order gram | obs_obs | obs_state | (masked:
the Dy per-component grams) | counts (16) | next_next | next_prev | prev_prev.  `statistics_step` is one launch's contribution
in that layout, `name_statistics` the map from two such arrays to the table above.

Tolerance.  A statistic is a plain sum of n float64 terms (n = trajectories x steps that contribute), each formed with at most
two roundings, so in ANY order its error is at most (n + 4) 2^-53 sum |term|; `statistics_step` returns sum |term| beside the
sum and `statistics_step_bound` the bound.  Kernel and contract each sum in their own order: kernel against contract is
allowed TWICE the bound, nothing more.
"""
import numpy as np

UNIT = 2.0 ** -53
ROWS = 16
PARAMETERS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
FLAG_INDEX_OUT_OF_RANGE = 4


def tri(n):
    return n * (n + 1) // 2


def layout(D, Dy, masked):
    """name -> slice of the [16, F] array's columns, and "columns": F (aesmc_switching_statistics_columns)."""
    X = D + 1
    sizes = [("gram", tri(X)), ("obs_obs", Dy), ("obs_state", Dy * X)] + ([("grams", Dy * tri(X))] if masked else []) + \
        [("counts", ROWS), ("next_next", tri(D)), ("next_prev", D * X), ("prev_prev", tri(X))]
    out, at = {}, 0
    for name, size in sizes:
        out[name] = slice(at, at + size)
        at += size
    out["columns"] = at
    return out


def pack(full):
    """[..., n, n] -> the packed lower triangles [..., n (n + 1) / 2]."""
    rows, cols = np.tril_indices(full.shape[-1])
    return full[..., rows, cols]


def unpack(packed, n):
    rows, cols = np.tril_indices(n)
    full = np.zeros(packed.shape[:-1] + (n, n))
    full[..., rows, cols] = packed
    full[..., cols, rows] = packed
    return full


def _gram(mean, cov, D):
    """E[x x^T] [..., X, X] of x = (z, 1), z ~ N(mean, unpack(cov))."""
    X = D + 1
    value = np.zeros(mean.shape[:-1] + (X, X))
    value[..., :D, :D] = unpack(cov, D) + mean[..., :, None] * mean[..., None, :]
    value[..., :D, D] = value[..., D, :D] = mean
    value[..., D, D] = 1.0
    return value


def _payload(y, regime, mean, cov, M, previous, observed):
    """([B,N,F] what each trajectory adds to its regime's row, whether it counts [B,N], flags)."""
    y = np.asarray(y, dtype=np.float64)
    regime, mean, cov = np.asarray(regime), np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    B, N, D = mean.shape
    Dy, X = y.shape[1], D + 1
    masked = observed is not None
    where = layout(D, Dy, masked)
    seen = np.ones((B, Dy), dtype=bool) if observed is None else np.asarray(observed).astype(bool)
    y = np.where(seen, y, 0.0)      # (y at an unobserved position is never used)
    counts = (regime >= 0) & (regime < M)
    out = np.zeros((B, N, where["columns"]))
    gram = _gram(mean, cov, D)
    x = np.concatenate([mean, np.ones((B, N, 1))], axis=-1)
    out[..., where["gram"]] = pack(gram)
    out[..., where["obs_obs"]] = (y * y)[:, None, :]
    out[..., where["obs_state"]] = (y[:, None, :, None] * x[:, :, None, :]).reshape(B, N, Dy * X)
    if masked:
        out[..., where["grams"]] = (seen[:, None, :, None] * pack(gram)[:, :, None, :]).reshape(B, N, -1)
    if previous is not None:
        regime_prev, mean_prev, cov_prev, cross = (np.asarray(value) for value in previous)
        counts &= (regime_prev >= 0) & (regime_prev < M)
        out[..., where["counts"]] = regime_prev[..., None] == np.arange(ROWS)
        out[..., where["next_next"]] = pack(gram[..., :D, :D])
        lagged = np.concatenate([cross + mean[..., :, None] * mean_prev[..., None, :], mean[..., :, None]], axis=-1)
        out[..., where["next_prev"]] = lagged.reshape(B, N, D * X)
        out[..., where["prev_prev"]] = pack(_gram(np.asarray(mean_prev, dtype=np.float64), cov_prev, D))
    return out, counts, 0 if counts.all() else FLAG_INDEX_OUT_OF_RANGE


def statistics_step(y, regime, mean, cov, M, previous=None, observed=None):
    """One launch's contribution (K45; with `observed` [B,Dy] bool, K46): (stats [16,F], sum of |term| [16,F], flags).
    y [B,Dy]; regime int [B,N]; mean [B,N,D], cov [B,N,D(D+1)/2]: the smoothed moments of z_t; previous: None (the t = 0 form:
    the transition block stays zero) or (regime_prev [B,N], mean_prev, cov_prev, cross [B,N,D,D]).  A trajectory whose regime
    or previous regime is outside [0, M) contributes nothing and raises FLAG_INDEX_OUT_OF_RANGE."""
    payload, counts, flags = _payload(y, regime, mean, cov, M, previous, observed)
    stats, magnitude = np.zeros((ROWS, payload.shape[-1])), np.zeros((ROWS, payload.shape[-1]))
    regime = np.asarray(regime)
    for j in range(min(M, ROWS)):
        rows = payload[counts & (regime == j)]
        stats[j], magnitude[j] = rows.sum(axis=0), np.abs(rows).sum(axis=0)
    return stats, magnitude, flags


def statistics_step_bound(y, regime, mean, cov, M, previous=None, observed=None, launches=1):
    """(n + 4) 2^-53 sum |term| per entry of `statistics_step`'s array, n = B N trajectories (times `launches` for a sum of
    that many launches whose magnitudes the caller adds): what ANY order of summation stays within.  Kernel against
    contract: twice this."""
    _, magnitude, _ = statistics_step(y, regime, mean, cov, M, previous, observed)
    terms = np.asarray(regime).size * launches
    return (terms + 4) * UNIT * magnitude


def name_statistics(initial, later, M, D, Dy, masked):
    """The table of the module's docstring from the two [16, F] blocks (t = 0, and the sum of the later steps)."""
    X = D + 1
    where = layout(D, Dy, masked)
    total = initial + later
    gram = unpack(total[:M, where["gram"]], X)
    if masked:
        grams = unpack(total[:M, where["grams"]].reshape(M, Dy, tri(X)), X)
    else:
        grams = np.broadcast_to(gram[:, None], (M, Dy, X, X))
    first = unpack(initial[:M, where["gram"]], X)
    return {"transition_counts": later[:M, where["counts"]][:, :M].T.copy(),
            "next_next": unpack(later[:M, where["next_next"]], D),
            "next_prev": later[:M, where["next_prev"]].reshape(M, D, X),
            "prev_prev": unpack(later[:M, where["prev_prev"]], X),
            "obs_obs": total[:M, where["obs_obs"]],
            "obs_state": total[:M, where["obs_state"]].reshape(M, Dy, X),
            "state_state": grams,
            "initial_counts": first[:, D, D].copy(),
            "initial_state": first.sum(axis=0)}


def expected_statistics(smoothed, observations, M, observed=None):
    """The whole pass: `statistics_step` at t = 0 into the initial block and at t >= 1 summed into the later one, named.
    smoothed: a dict with regimes (T x [B,N]), means, covariances (T each) and cross_covariances (T-1); observations T x [B,Dy];
    observed: None or T entries, each None or bool [B,Dy].  Returns the named statistics with batch_size, num_trajectories,
    num_timesteps, flags and `bounds`: name -> the array of (n + 4) 2^-53 sum |term| (n = the trajectories times the steps
    that contribute to that statistic)."""
    regimes, means, covs, crosses = (smoothed[key] for key in ("regimes", "means", "covariances", "cross_covariances"))
    T = len(observations)
    B, N, D = np.asarray(means[0]).shape
    Dy = np.asarray(observations[0]).shape[1]
    masked = observed is not None
    mask = lambda t: None if not masked else (np.ones((B, Dy), dtype=bool) if observed[t] is None else observed[t])
    initial, initial_mag, flags = statistics_step(observations[0], regimes[0], means[0], covs[0], M, None, mask(0))
    later, later_mag = np.zeros_like(initial), np.zeros_like(initial)
    for t in range(1, T):
        step, mag, bits = statistics_step(observations[t], regimes[t], means[t], covs[t], M,
                                          (regimes[t - 1], means[t - 1], covs[t - 1], crosses[t - 1]), mask(t))
        later, later_mag, flags = later + step, later_mag + mag, flags | bits
    out = name_statistics(initial, later, M, D, Dy, masked)
    magnitudes = name_statistics(initial_mag, later_mag, M, D, Dy, masked)
    steps = {"initial_counts": 1, "initial_state": 1, "obs_obs": T, "obs_state": T, "state_state": T}
    out["bounds"] = {name: (B * N * steps.get(name, T - 1) + 4) * UNIT * magnitudes[name] for name in magnitudes}
    out.update(batch_size=B, num_trajectories=N, num_timesteps=T, flags=flags)
    return out


def brute_force_statistics(smoothed, observations, M, observed=None):
    """The same named statistics by three nested loops over (t, b, n) on dense matrices: the independent side."""
    regimes, means, covs, crosses = (smoothed[key] for key in ("regimes", "means", "covariances", "cross_covariances"))
    T = len(observations)
    B, N, D = np.asarray(means[0]).shape
    Dy, X = np.asarray(observations[0]).shape[1], D + 1
    out = {"transition_counts": np.zeros((M, M)), "next_next": np.zeros((M, D, D)), "next_prev": np.zeros((M, D, X)),
           "prev_prev": np.zeros((M, X, X)), "obs_obs": np.zeros((M, Dy)), "obs_state": np.zeros((M, Dy, X)),
           "state_state": np.zeros((M, Dy, X, X)), "initial_counts": np.zeros(M), "initial_state": np.zeros((X, X))}

    def moments(t, b, n):
        m = np.asarray(means[t])[b, n]
        P = unpack(np.asarray(covs[t])[b, n], D)
        x = np.append(m, 1.0)
        second = np.outer(x, x)
        second[:D, :D] += P
        return m, x, second

    for t in range(T):
        for b in range(B):
            for n in range(N):
                j = int(np.asarray(regimes[t])[b, n])
                m, x, second = moments(t, b, n)
                for c in range(Dy):
                    if observed is not None and observed[t] is not None and not observed[t][b, c]:
                        continue
                    value = float(np.asarray(observations[t])[b, c])
                    out["obs_obs"][j, c] += value * value
                    out["obs_state"][j, c] += value * x
                    out["state_state"][j, c] += second
                if t == 0:
                    out["initial_counts"][j] += 1.0
                    out["initial_state"] += second
                    continue
                i = int(np.asarray(regimes[t - 1])[b, n])
                m_prev, x_prev, second_prev = moments(t - 1, b, n)
                out["transition_counts"][i, j] += 1.0
                out["next_next"][j] += second[:D, :D]
                lagged = np.outer(m, x_prev)
                lagged[:, :D] += np.asarray(crosses[t - 1])[b, n]
                out["next_prev"][j] += lagged
                out["prev_prev"][j] += second_prev
    return out


# ---- the M-step and the score ------------------------------------------------------------------------------------------------------

def _regress(cross, gram, weights, free):
    """Row-wise least squares W gram = cross in the columns `free` (bool [X]) with the others held at `weights`."""
    fixed = ~free
    target = cross[..., free] - weights[..., fixed] @ gram[..., fixed, :][..., :, free]
    out = weights.copy()
    out[..., free] = target @ np.linalg.pinv(gram[..., free, :][..., :, free], hermitian=True)
    return out


def _quadratic(square, cross, gram, weights):
    """square - 2 w . cross + w gram w^T per row w of `weights`: [..., rows] from [..., rows], [..., rows, X], [..., X, X]
    (or a gram per row, [..., rows, X, X])."""
    if gram.ndim == weights.ndim:
        gram = gram[..., None, :, :]
    return square - 2.0 * (weights * cross).sum(axis=-1) + np.einsum("...i,...il,...l->...", weights, gram, weights)


def _affine_update(prev_w, prev_b, prev_scale, square, cross, gram, count, learn_w, learn_b, learn_scale, names):
    """One affine-Gaussian block (transition: rows of [A b] with q; emission: rows of [C d] with r).  square [M,R],
    cross [M,R,X], gram [M,X,X] or [M,R,X,X], count [M] or [M,R]: the statistics; returns (w, b, scale) in the shapes of the
    previous ones.  A leading extent of 1 pools the statistics over the regimes."""
    M, R, X = cross.shape
    if gram.ndim == 3:
        gram = np.broadcast_to(gram[:, None], (M, R, X, X))
    if count.ndim == 1:
        count = np.broadcast_to(count[:, None], (M, R))
    if prev_w.shape[0] != prev_b.shape[0]:
        raise NotImplementedError("m_step: {} and {} must both be shared across regimes or neither".format(*names[:2]))
    pool = lambda value, shared: value.sum(axis=0, keepdims=True) if shared and M > 1 else value
    w_shared, s_shared = prev_w.shape[0] == 1 and M > 1, prev_scale.shape[0] == 1 and M > 1
    weights = np.concatenate([prev_w, prev_b[..., None]], axis=-1)
    if learn_w or learn_b:
        free = np.array([learn_w] * (X - 1) + [learn_b])
        visited = pool(count, w_shared) > 0
        solved = _regress(pool(cross, w_shared)[..., None, :], pool(gram, w_shared), weights[..., None, :], free)[..., 0, :]
        weights = np.where(visited[..., None], solved, weights)
    new_scale = prev_scale
    if learn_scale:
        full = np.broadcast_to(weights, (M, R, X))
        quad, total = pool(_quadratic(square, cross, gram, full), s_shared), pool(count, s_shared)
        with np.errstate(invalid="ignore", divide="ignore"):
            estimate = np.sqrt(np.maximum(quad, 0.0) / total)
        new_scale = np.where(total > 0, estimate, prev_scale)
    return weights[..., :-1], weights[..., -1], new_scale


def m_step(stats, previous, learn=PARAMETERS):
    """The closed-form M-step: a new model (a dict of the ten arrays, each in `previous`'s shape) that maximises the expected
    complete-data log-likelihood the statistics stand for, in the parameters named by `learn`; the rest is copied.

    pi0 = initial_counts / (B N); Pi's rows from transition_counts (a row with no departures keeps the previous one); m0 and
    s0 from initial_state; [A_j b_j] = next_prev[j] pinv(prev_prev[j]); q_ji^2 = (next_next_ii - 2 w . next_prev_i + w prev_prev
    w^T) / n_j with w = [A_j b_j]_i (clamped at 0); row c of [C_j d_j] and r_jc the same regression on obs_state, state_state
    [:, c] and obs_obs.  With only one of A, b (C, d) learned the other is held at its previous value in the regression.  A
    regime never visited keeps its previous block, and so does a component never observed under a regime.  A leading extent
    of 1 (shared across regimes) is estimated from the statistics summed over the regimes and keeps that shape."""
    unknown = sorted(set(learn) - set(PARAMETERS))
    if unknown:
        raise ValueError("m_step: learn names {} — the parameters are {}".format(unknown, PARAMETERS))
    new = {name: np.array(previous[name], dtype=np.float64) for name in PARAMETERS}
    D = new["A"].shape[-1]
    if "pi0" in learn:
        new["pi0"] = stats["initial_counts"] / (stats["batch_size"] * stats["num_trajectories"])
    if "Pi" in learn:
        departures = stats["transition_counts"].sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            new["Pi"] = np.where(departures > 0, stats["transition_counts"] / departures, new["Pi"])
    first = stats["initial_state"]
    if first[D, D] > 0:
        if "m0" in learn:
            new["m0"] = first[:D, D] / first[D, D]
        if "s0" in learn:
            m0 = new["m0"]
            quad = np.maximum(np.diag(first)[:D] - 2.0 * m0 * first[:D, D] + m0 * m0 * first[D, D], 0.0)
            shape = new["s0"].shape
            new["s0"] = (np.sqrt(quad / first[D, D]) if new["s0"].size == D else
                         np.sqrt(quad.sum() / (D * first[D, D])) * np.ones(1)).reshape(shape)
    lagged = stats["prev_prev"]
    new["A"], new["b"], new["q"] = _affine_update(
        new["A"], new["b"], new["q"], np.diagonal(stats["next_next"], axis1=-2, axis2=-1), stats["next_prev"], lagged,
        lagged[:, D, D], "A" in learn, "b" in learn, "q" in learn, ("A", "b", "q"))
    grams = stats["state_state"]
    new["C"], new["d"], new["r"] = _affine_update(
        new["C"], new["d"], new["r"], stats["obs_obs"], stats["obs_state"], grams, grams[:, :, D, D], "C" in learn,
        "d" in learn, "r" in learn, ("C", "d", "r"))
    return new


def _affine_score(w, b, scale, square, cross, gram, count, N):
    M, R, X = cross.shape
    if gram.ndim == 3:
        gram = np.broadcast_to(gram[:, None], (M, R, X, X))
    if count.ndim == 1:
        count = np.broadcast_to(count[:, None], (M, R))
    weights = np.broadcast_to(np.concatenate([np.broadcast_to(w, (M,) + w.shape[1:]),
                                              np.broadcast_to(b, (M,) + b.shape[1:])[..., None]], axis=-1), (M, R, X))
    sigma = np.broadcast_to(scale, (M, R))
    residual = (cross - np.einsum("mrl,mrlk->mrk", weights, gram)) / (sigma * sigma)[..., None] / N
    quad = _quadratic(square, cross, gram, weights)
    grad_scale = (-count / sigma + quad / sigma ** 3) / N
    fold = lambda grad, like: grad.sum(axis=0, keepdims=True) if like.shape[0] == 1 and M > 1 else grad
    return fold(residual[..., :-1], w), fold(residual[..., -1], b), fold(grad_scale, scale)


def score(stats, model):
    """Fisher's identity: the gradient, with respect to each of the model's ten arrays in the array's own shape, of the Monte
    Carlo estimate of sum_b log p(y^b), (1/N) sum_{b,n} E[grad log p(y^b, z, s^{b,n}) | y^b, s^{b,n}].  For [A b]:
    diag(q_j^-2) (next_prev[j] - [A_j b_j] prev_prev[j]) / N; for q: (-n_j / q + quadratic / q^3) / N; likewise C, d, r, m0,
    s0; for Pi and pi0 the plain partial derivatives count / probability (0 where the count is 0; the simplex is the
    caller's business).  A parameter shared across regimes (leading extent 1) receives the sum over the regimes."""
    model = {name: np.asarray(model[name], dtype=np.float64) for name in PARAMETERS}
    N = stats["num_trajectories"]
    D = model["A"].shape[-1]
    out = {}
    lagged = stats["prev_prev"]
    out["A"], out["b"], out["q"] = _affine_score(model["A"], model["b"], model["q"],
                                                 np.diagonal(stats["next_next"], axis1=-2, axis2=-1), stats["next_prev"],
                                                 lagged, lagged[:, D, D], N)
    grams = stats["state_state"]
    out["C"], out["d"], out["r"] = _affine_score(model["C"], model["d"], model["r"], stats["obs_obs"], stats["obs_state"],
                                                 grams, grams[:, :, D, D], N)
    first = stats["initial_state"]
    m0, s0 = model["m0"], np.broadcast_to(model["s0"].reshape(-1), (D,))
    out["m0"] = (first[:D, D] - m0 * first[D, D]) / (s0 * s0) / N
    quad = np.diag(first)[:D] - 2.0 * m0 * first[:D, D] + m0 * m0 * first[D, D]
    grad_s0 = (-first[D, D] / s0 + quad / s0 ** 3) / N
    out["s0"] = (grad_s0 if model["s0"].size == D else grad_s0.sum() * np.ones(1)).reshape(model["s0"].shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["Pi"] = np.where(stats["transition_counts"] > 0, stats["transition_counts"] / model["Pi"], 0.0) / N
        out["pi0"] = np.where(stats["initial_counts"] > 0, stats["initial_counts"] / model["pi0"], 0.0) / N
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def example_step(B, N, M, D, Dy, observation_dtype=np.float64, seed=0):
    """(y [B,Dy], regime [B,N] int32, mean, cov, previous = (regime_prev, mean_prev, cov_prev, cross)) of one launch: random
    regimes in [0, M), standard-normal means and observations, covariances F F^T / D + 0.1 I (packed), cross-covariances
    0.3 N(0, 1)."""
    rng = np.random.default_rng([seed, B, N, M, D, Dy, 45])

    def moments():
        factor = rng.standard_normal((B, N, D, D))
        return rng.standard_normal((B, N, D)), pack(factor @ np.swapaxes(factor, -1, -2) / D + 0.1 * np.eye(D))

    regime, regime_prev = (rng.integers(0, M, size=(B, N)).astype(np.int32) for _ in range(2))
    mean, cov = moments()
    mean_prev, cov_prev = moments()
    cross = 0.3 * rng.standard_normal((B, N, D, D))
    y = rng.standard_normal((B, Dy)).astype(observation_dtype)
    return y, regime, mean, cov, (regime_prev, mean_prev, cov_prev, cross)


def example_smoothed(B, N, M, D, Dy, T, seed=0):
    """(smoothed, observations) of a whole pass on made-up moments: `example_step`'s per timestep — regimes, means,
    covariances (T each) and cross_covariances (T-1), with observations T x [B,Dy].  Nothing here is a smoother's output: the
    statistics are sums of whatever moments they are given."""
    steps = [example_step(B, N, M, D, Dy, seed=1000 * seed + t) for t in range(T)]
    smoothed = {"regimes": [step[1] for step in steps], "means": [step[2] for step in steps],
                "covariances": [step[3] for step in steps], "cross_covariances": [step[4][3] for step in steps[1:]]}
    return smoothed, [step[0] for step in steps]
