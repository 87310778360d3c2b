"""TEST INFRASTRUCTURE: the contract of the two first-generation reductions over particles, in NumPy float64, with the
inputs under which every particle of a row counts.

  * K1 (include/aesmc_hip.h: aesmc_logweight_lse, aesmc_logweight_accumulate, aesmc_logweight_lse_backward);
  * K7 (aesmc_particle_summary).

Written independently of the kernels' parallel structure: one maximum per row, one sum in NumPy's order.  The `*_bound`
functions say how far a float64 evaluation in ANOTHER order (lanes, slices, running maxima that are rescaled) may lie
from these; they are derived, not measured, and zero where the result is a convention.

The sums the kernels form are sums of K non-negative terms e_k = exp(lw_k - m) (times |v_k| or v_k^2 under the magnitude
the metric divides by).  Any order of the K additions moves such a sum by at most eps64 * (K - 1) of itself; the
exponential and the subtraction in front of it move a term that matters (lw_k - m >= -40: the rest carry K e^-40 of the
sum) by 40 eps for the rounded difference plus a few eps for exp; a rescale by exp(m' - m) of a partial sum is one more
such factor per level of the merge (lane, wavefront, workgroup, slice: four).  SLACK = 96 covers these with room.
"""
import numpy as np

EPSILON = 2.0 ** -52
SLACK = 96
REST = -1e4            # exp(REST - m) is exactly 0 in float32 and float64 for every m >= -9000
PROBES = (0, 63, 64, 255, 256)        # and K - 1: both sides of a wavefront's and of a 256-particle tile's edge


# ---- K1 -----------------------------------------------------------------------------------------------------------------
def row_lse(lw):
    """float64 [B]: log sum_k exp(lw[b,k]) with the conventions of include/aesmc_hip.h (torch.logsumexp's): a NaN anywhere
    in the row -> NaN; else a +inf anywhere -> +inf; a row of -inf (or without particles) -> -inf."""
    lw = np.asarray(lw, dtype=np.float64)
    B, K = lw.shape
    out = np.full(B, -np.inf)
    if K == 0:
        return out
    with np.errstate(all="ignore"):
        m = lw.max(axis=1)                                   # NaN propagates through np.max
        finite = np.isfinite(m)
        shift = np.where(finite, m, 0.0)
        s = np.exp(lw - shift[:, None]).sum(axis=1)
        out = np.where(finite, shift + np.log(s), m)         # m is NaN, +inf or -inf where it is not finite
        out = np.where(np.isnan(lw).any(axis=1), np.nan, out)
    return out


def logweight_lse(a, b=None, c=None):
    """K1: lw = a + b - c in the INPUT dtype (two IEEE operations, left to right: held bit for bit), and the float64
    log-sum-exp over particles of that rounded lw.  Returns (lw, lse float64 [B])."""
    a = np.asarray(a)
    with np.errstate(all="ignore"):
        lw = np.array(a, copy=True)
        if b is not None:
            lw = (lw + np.asarray(b, dtype=a.dtype)).astype(a.dtype)
        if c is not None:
            lw = (lw - np.asarray(c, dtype=a.dtype)).astype(a.dtype)
    return lw, row_lse(lw)


def logweight_accumulate(a, b, c, acc):
    """K1 with the running sum: lw as above, total = acc + lw in the input dtype (acc first), lse of total.
    Returns (lw, total, lse float64)."""
    lw, _ = logweight_lse(a, b, c)
    with np.errstate(all="ignore"):
        total = (np.asarray(acc, dtype=lw.dtype) + lw).astype(lw.dtype)
    return lw, total, row_lse(total)


def lse_bound(lw):
    """float64 [B], absolute: eps64 * (K + SLACK) for the sum under the logarithm (see the module's docstring) plus
    2 eps64 |lse| for the maximum added back (once in a lane's pair, once at the end).  Zero where lse is not finite."""
    lw = np.asarray(lw, dtype=np.float64)
    lse = row_lse(lw)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(lse), EPSILON * (lw.shape[1] + SLACK + 2.0 * np.abs(np.where(np.isfinite(lse), lse, 0.0))), 0.0)


def logweight_lse_backward(lw, lse, grad_lw=None, grad_lse=None):
    """K1 backward in float64: g[b,k] = grad_lse[b] * exp(lw[b,k] - lse[b]) + grad_lw[b,k]; either gradient may be None
    (its term is dropped, not multiplied by zero).  `lse` is DATA: the kernel reads it and does not form it.  Where lse is
    not finite the expression is evaluated as written, which the kernel does too: lse = -inf gives exp(lw + inf) (+inf, or
    NaN where lw = -inf) times grad_lse; lse = +inf gives 0 for lw < +inf and NaN where lw = +inf; NaN gives NaN.
    Returns (g, -g)."""
    lw = np.asarray(lw, dtype=np.float64)
    g = np.zeros_like(lw)
    with np.errstate(all="ignore"):
        if grad_lse is not None:
            g = np.asarray(grad_lse, dtype=np.float64)[:, None] * np.exp(lw - np.asarray(lse, dtype=np.float64)[:, None])
        if grad_lw is not None:
            g = g + np.asarray(grad_lw, dtype=np.float64)
    return g, -g


def backward_scale(lw, lse, grad_lw=None, grad_lse=None):
    """[B,K] float64: |grad_lse| exp(lw - lse) + |grad_lw|, the size of a particle's own gradient (the metric's
    denominator; where it is 0 the gradient is exactly 0)."""
    lw = np.asarray(lw, dtype=np.float64)
    scale = np.zeros_like(lw)
    with np.errstate(all="ignore"):
        if grad_lse is not None:
            scale = np.abs(np.asarray(grad_lse, dtype=np.float64))[:, None] * np.exp(lw - np.asarray(lse, dtype=np.float64)[:, None])
        if grad_lw is not None:
            scale = scale + np.abs(np.asarray(grad_lw, dtype=np.float64))
    return scale


def backward_bound(lw, lse):
    """[B,K] float64, RELATIVE to `backward_scale`: nothing is summed, so what moves is the rounded difference in front
    of exp (eps64 |lw - lse| in the exponent, that factor on the term), exp itself, the product and the addition:
    eps64 * (|lw - lse| + 8).  Zero where lw - lse is not finite (conventions, held exactly)."""
    with np.errstate(all="ignore"):
        d = np.asarray(lw, dtype=np.float64) - np.asarray(lse, dtype=np.float64)[:, None]
    return np.where(np.isfinite(d), EPSILON * (np.abs(np.where(np.isfinite(d), d, 0.0)) + 8.0), 0.0)


# ---- K7 -----------------------------------------------------------------------------------------------------------------
def _weights(log_w):
    lw = np.asarray(log_w, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = lw.max(axis=1, keepdims=True) if lw.shape[1] else np.full((lw.shape[0], 1), np.nan)
        broken = ~np.isfinite(m[:, 0])                        # NaN, +inf, or nothing but -inf
        e = np.exp(lw - np.where(broken[:, None], 0.0, m))
        e[broken] = np.nan
    return e, broken


def particle_summary(log_w, value=None):
    """K7 in float64: (log_ess [B], mean [B,...], second moment [B,...]) under w = softmax(log_w, axis=1); mean and second
    are None without `value`.  log_ess = 2 log sum e - log sum e^2 with e = exp(lw - max): the maximum cancels, so offsets
    cost no digits.  Rows whose weights cannot be normalised (a NaN, a +inf, nothing but -inf) give NaN everywhere, as the
    reference's softmax does.  (The oracle module of the older tests calls this function: one definition.)"""
    e, broken = _weights(log_w)
    B, K = e.shape
    with np.errstate(all="ignore"):
        s1, s2 = e.sum(axis=1), (e * e).sum(axis=1)
        log_ess = np.where(broken, np.nan, 2 * np.log(s1) - np.log(s2))
        mean = second = None
        if value is not None:
            v = np.asarray(value, dtype=np.float64)
            w = (e / s1[:, None]).reshape((B, K) + (1,) * (v.ndim - 2))
            mean, second = (w * v).sum(axis=1), (w * v * v).sum(axis=1)
            mean[broken] = np.nan
            second[broken] = np.nan
    return log_ess, mean, second


def summary_magnitudes(log_w, value):
    """(sum_k w_k |v_k|, sum_k w_k v_k^2), each [B,...] float64: what the metric divides the error of the mean and of the
    second moment by.  Zero on rows whose weights cannot be normalised."""
    e, broken = _weights(log_w)
    v = np.asarray(value, dtype=np.float64)
    B, K = e.shape
    with np.errstate(all="ignore"):
        w = (e / e.sum(axis=1)[:, None]).reshape((B, K) + (1,) * (v.ndim - 2))
        first, second = (w * np.abs(v)).sum(axis=1), (w * v * v).sum(axis=1)
    first[broken] = 0.0
    second[broken] = 0.0
    return first, second


def log_ess_bound(log_w):
    """float64 [B], absolute: three sums' worth (2 log sum e, log sum e^2) of eps64 * (K + SLACK).  Zero on broken rows."""
    e, broken = _weights(log_w)
    return np.where(broken, 0.0, 3.0 * EPSILON * (e.shape[1] + SLACK))


def summary_bound(log_w):
    """float64 [B], RELATIVE to `summary_magnitudes` (both moments alike): numerator and normaliser are each a sum of K
    non-negative terms under the magnitude, eps64 * (K + SLACK) apiece; v^2 costs one rounding more, inside SLACK.
    Zero on broken rows."""
    e, broken = _weights(log_w)
    return np.where(broken, 0.0, 2.0 * EPSILON * (e.shape[1] + SLACK))


def values(B, K, tail):
    """value[b,k,j] = (31 k + 7 j + b) % 251 - 125 (float64, j the flat index of the trailing dims): distinct small
    integers, exact in float32 with their squares, so a particle read from the wrong address is a different number."""
    D = int(np.prod(tail)) if len(tail) else 1
    b, k, j = np.meshgrid(np.arange(B), np.arange(K), np.arange(D), indexing="ij")
    return ((31 * k + 7 * j + b) % 251 - 125).astype(np.float64).reshape((B, K) + tuple(tail))


# ---- weight profiles: functions of (B, K, dtype, seed) -> [B,K] of `dtype` ---------------------------------------------------
def effective_sample_size(lw):
    e, _ = _weights(lw)
    with np.errstate(all="ignore"):
        return e.sum(axis=1) ** 2 / (e * e).sum(axis=1)


def assert_flat(lw):
    ess, K = effective_sample_size(lw), np.asarray(lw).shape[1]
    assert float(ess.min()) >= K / 4.0, "weights too peaked for this check: ESS {} of {} particles".format(float(ess.min()), K)


def _flat_rows(B, K, dtype, seed, shift=0.0):
    """randn + shift rounded to `dtype`; rows whose effective sample size is below K / 4 are drawn again, alone (at most
    32 times), so one peaked row in hundreds does not discard the others."""
    lw = (np.random.RandomState(seed).randn(B, K) + shift).astype(dtype)
    for attempt in range(1, 33):
        peaked = np.flatnonzero(effective_sample_size(lw) < K / 4.0)
        if len(peaked) == 0:
            break
        lw[peaked] = (np.random.RandomState(seed + 7919 * attempt).randn(len(peaked), K) + shift).astype(dtype)
    assert_flat(lw)
    return lw


def flat(B, K, dtype, seed):
    """randn: an effective sample size near K / e, asserted >= K / 4 in every row."""
    return _flat_rows(B, K, dtype, seed)


def wide(B, K, dtype, seed):
    """10 randn: eighty units between the ends of a row; a handful of particles hold the weight.  In float32 clipped at
    +-36, so that exp(lw - lse) >= e^-81 stays a normal number (a subnormal carries few bits, and the per-particle metric
    of the backward has no floor)."""
    lw = 10.0 * np.random.RandomState(seed).randn(B, K)
    if np.dtype(dtype) == np.float32:
        lw = np.clip(lw, -36.0, 36.0)
    return lw.astype(dtype)


def minus_inf_stretch(B, K, dtype, seed):
    """`flat` with the particles [K/4, K/4 + K/2) of every row at -inf (zero weight is legal: aesmc/inference.py:253)."""
    lw = flat(B, K, dtype, seed)
    lw[:, K // 4: K // 4 + K // 2] = -np.inf
    return lw


def dominant_position(b, K):
    return K - 1 - (7 * b) % max(1, K // 4)


def dominant(B, K, dtype, seed):
    """`flat` plus 60 on one particle in the last quarter of the row: every partial maximum before it is overtaken."""
    lw = flat(B, K, dtype, seed).astype(np.float64)
    for b in range(B):
        lw[b, dominant_position(b, K)] += 60.0
    return lw.astype(dtype)


def ascending(B, K, dtype, seed=0, reverse=False):
    """lw[b,k] = (k + b) * delta with delta = 1 / 128 (exact in float32 for every k here, and 8192 particles span 64
    units: exp(lw - lse) stays a normal float32): each value is larger than all before it, so a running maximum moves at
    EVERY push of every lane; `reverse` runs downhill (it never moves)."""
    lw = ((np.arange(K)[None, :] + np.arange(B)[:, None]) / 128.0)
    return (lw[:, ::-1] if reverse else lw).astype(dtype).copy()


def descending(B, K, dtype, seed=0):
    return ascending(B, K, dtype, seed, reverse=True)


def offset(B, K, dtype, seed, sign=+1):
    """`flat` moved by +-1e6 (float64) or +-1e4 (float32), rounded to the dtype AFTER the move (the spacing of the dtype
    there is what the row then has); still asserted flat.  lse itself is then +-1e6: under a metric relative to |lse| no
    single particle shows, so K1's tests also run these rows through `logweight_accumulate` with -+shift as the running
    sum, whose total is a flat row again (the subtraction is exact); K7's log_ess is free of the offset."""
    return _flat_rows(B, K, dtype, seed, sign * offset_shift(dtype))


def offset_shift(dtype):
    return 1e6 if np.dtype(dtype) == np.float64 else 1e4


def offset_up(B, K, dtype, seed):
    return offset(B, K, dtype, seed, +1)


def offset_down(B, K, dtype, seed):
    return offset(B, K, dtype, seed, -1)


def probe_positions(K, L=None):
    """{0, 63, 64, 255, 256, K-1} and, given a slice length L, {L-1, L, 2L-1, 2L}; those inside the row, sorted."""
    at = set(PROBES) | {K - 1}
    if L:
        at |= {L - 1, L, 2 * L - 1, 2 * L}
    return sorted(p for p in at if 0 <= p < K)


def probes(B, K, dtype, seed=0, L=None, rest=REST):
    """Weight 0 at `probe_positions(K, L)`, every other particle at `rest` (-1e4: exp underflows to exactly 0 in both
    dtypes; -inf: whole slices then hold no usable maximum).  The weights are exactly 1 / #probes."""
    lw = np.full((B, K), rest, dtype=np.float64)
    lw[:, probe_positions(K, L)] = 0.0
    return lw.astype(dtype)


def one_hot(B, K, dtype, positions, rest=REST):
    """Row b: particle positions[b] at 0.5 + b, the rest at `rest`.  Every output is then exact: lse = 0.5 + b,
    log_ess = 0, mean = value[b,p], second = value[b,p]^2, g[b,p] = grad_lse[b] and 0 elsewhere."""
    lw = np.full((B, K), rest, dtype=np.float64)
    for b, p in enumerate(positions):
        lw[b, p] = 0.5 + b
    return lw.astype(dtype)


# ---- mutations: the same contract, deliberately wrong (tests/test_reductions_contract.py) ----------------------------------
COUNTED = 1.25e-4


def counted_share(K):
    """A particle (or slice) counts when it holds at least max(1 / (2 K), 1.25e-4) of its row's weight: leaving it out
    moves log sum e by -log(1 - w) >= w, counting it twice by log(1 + w) >= w - w^2 / 2, both >= 1e-4.  What holds less
    cannot show in a row sum at that size under any metric; the one-hot sweeps are there for those."""
    return max(0.5 / K, COUNTED)


def centred(lw):
    """lw minus the integer nearest to its row's log-sum-exp (rounded to lw's dtype again): |lse| <= 1/2 afterwards, so
    the metric |got - want| / max(1, |want|) of lse is an absolute one and a particle's share shows undivided.  Rows
    without a finite lse are left as they are."""
    lse = row_lse(lw)
    shift = np.where(np.isfinite(lse), np.rint(np.where(np.isfinite(lse), lse, 0.0)), 0.0)
    with np.errstate(all="ignore"):
        return (np.asarray(lw, dtype=np.float64) - shift[:, None]).astype(np.asarray(lw).dtype)


def on_grid(x, step=2.0 ** -10):
    """x rounded to multiples of `step` (infinities kept), in x's dtype.  K1's backward reads lw and lse as data and forms
    lw - lse in their dtype: with both on this grid and below 2^13 in size the float32 difference is exact, so the one
    rounding every float32 evaluation shares (|lw - lse| eps32 / 2 on the exponent: 5e-6 of a particle eighty units down)
    stays out of the comparison with float64 and the rest — exp, the product, the sum — is measured alone."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(x), np.rint(x.astype(np.float64) / step) * step, x).astype(x.dtype)


def counted(lw):
    """bool [B,K]: particles that hold at least `counted_share(K)` of their row's weight."""
    e, broken = _weights(lw)
    with np.errstate(all="ignore"):
        w = e / e.sum(axis=1)[:, None]
    return np.where(broken[:, None], False, w >= counted_share(e.shape[1]))


def least_counted(lw, row=0):
    """The counted particle of `row` with the least weight (the one whose loss is hardest to see)."""
    e, _ = _weights(lw)
    held = np.where(counted(lw)[row], e[row], np.inf)
    return int(np.argmin(held))


def least_counted_slice(lw, L, row=0):
    """The slice [s L, (s+1) L) of `row` with the least weight among those that hold at least `counted_share(K)` of it."""
    e, _ = _weights(lw)
    K = e.shape[1]
    sums = np.array([e[row, s: s + L].sum() for s in range(0, K, L)])
    sums = np.where(sums >= counted_share(K) * e[row].sum(), sums, np.inf)
    return int(np.argmin(sums))


def drop_particle(lw, value, row, k):
    """The inputs on which the CORRECT contract returns what a kernel that left particle k of `row` out would."""
    lw = np.array(lw, copy=True)
    lw[row, k] = -np.inf
    return lw, value


def double_particle(lw, value, row, k):
    """... what a kernel that counted particle k of `row` twice would: the particle appended once more to every row (at
    -inf in the other rows)."""
    B, K = lw.shape
    extra = np.full((B, 1), -np.inf, dtype=lw.dtype)
    extra[row, 0] = lw[row, k]
    lw = np.concatenate([lw, extra], axis=1)
    if value is not None:
        value = np.concatenate([value, value[:, k: k + 1]], axis=1)
    return lw, value


def drop_slice(lw, value, row, s, L):
    """... what a kernel that left slice s (length L) of `row` out would."""
    lw = np.array(lw, copy=True)
    lw[row, s * L: (s + 1) * L] = -np.inf
    return lw, value
