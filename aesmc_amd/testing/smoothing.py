"""NumPy statement of the CONTRACT of the backward-simulation kernel (include/aesmc_hip.h, aesmc_backward_sample),
written without regard to the kernel's structure (no tiles, no chunks, no passes) — what the tests hold the HIP result to,
exactly — and of the whole backward pass that `aesmc_amd.smoothing.backward_simulate` makes of it.

One backward step of forward filtering / backward simulation (Godsill, Doucet & West 2004): trajectory m, whose state at
t+1 is target[b,m], draws particle k of step t with probability proportional to

    exp(log_w[b,k]) * Normal(target[b,m]; loc[b,k], scale)

by inverting the running sum of those weights at u[b,m].  (This package never imports the oracle — tests/test_library.py.)
"""
import numpy as np

FLAG_NAN_LOG_WEIGHT = 1
FLAG_DEGENERATE_ROW = 2

# below this the kernels' float64 exp of a non-positive number (csrc/ancestor_index.hpp) is zero
EXP_UNDERFLOW = -745.2


def backward_weights(log_w_row, loc_row, target_row, scale):
    """(w [M,K] float64, nan [M] bool, degenerate [M] bool) of one batch row: log_w_row [K], loc_row [K,D] or None,
    target_row [M,D] or None (then M comes from nowhere: pass a [M,0] array), scale [D] or one value."""
    lw = np.asarray(log_w_row).astype(np.float64)
    K = lw.shape[0]
    target = np.asarray(target_row)
    M, D = target.shape
    q = np.zeros((M, K), dtype=np.float64)
    if D:
        loc = np.asarray(loc_row).astype(np.float64)
        inv = 1.0 / np.broadcast_to(np.asarray(scale).astype(np.float64).reshape(-1), (D,))
        with np.errstate(invalid="ignore", over="ignore"):
            for d in range(D):
                q = q + ((target[:, d].astype(np.float64)[:, None] - loc[None, :, d]) * inv[d]) ** 2
    with np.errstate(invalid="ignore", over="ignore"):
        s = lw[None, :] - 0.5 * q
        nan = np.isnan(s).any(axis=1)
        smax = np.where(nan, 0.0, np.max(np.where(np.isnan(s), -np.inf, s), axis=1))
        degenerate = ~nan & ~np.isfinite(smax)
        x = s - np.where(nan | degenerate, 0.0, smax)[:, None]
        w = np.where(x > EXP_UNDERFLOW, np.exp(np.minimum(x, 0.0)), 0.0)
    return w, nan, degenerate


def backward_sample(log_w, loc, target, scale, u, payload=None):
    """log_w [B,K]; loc [B,K,D] / target [B,M,D] / scale (one value or [D]) or all three None (no transition term);
    u [B,M] float64 in [0, 1); payload [B,K,...] or None -> (idx int64 [B,M], flags, payload[b, idx[b,m]] or None).

        idx[b,m] = min( #{k : C[m,k] <= u[b,m] * C[m,K-1]},  max{k : w[m,k] > 0} ),   C = cumsum(w[m,:])

    A NaN among a trajectory's scores: FLAG_NAN_LOG_WEIGHT and idx = K; no finite maximum: FLAG_DEGENERATE_ROW and idx = K.
    The payload of idx == K is particle K-1's."""
    log_w = np.asarray(log_w)
    B, K = log_w.shape
    u = np.asarray(u, dtype=np.float64)
    M = u.shape[1]
    if u.shape != (B, M):
        raise ValueError("one uniform per trajectory: u must be [{}, M], got {}".format(B, u.shape))
    if loc is None:
        loc3, target3 = np.zeros((B, K, 0)), np.zeros((B, M, 0))
    else:
        loc3, target3 = np.asarray(loc).reshape(B, K, -1), np.asarray(target).reshape(B, M, -1)
    idx = np.empty((B, M), dtype=np.int64)
    flags = 0
    for b in range(B):
        w, nan, degenerate = backward_weights(log_w[b], loc3[b], target3[b], scale)
        if nan.any():
            flags |= FLAG_NAN_LOG_WEIGHT
        if degenerate.any():
            flags |= FLAG_DEGENERATE_ROW
        for m in range(M):
            if nan[m] or degenerate[m]:
                idx[b, m] = K
                continue
            c = np.cumsum(w[m])
            count = int(np.searchsorted(c, u[b, m] * c[-1], side="right"))
            idx[b, m] = min(count, int(np.flatnonzero(w[m] > 0)[-1]))
    moved = None
    if payload is not None:
        payload = np.asarray(payload)
        moved = np.stack([payload[b][np.minimum(idx[b], K - 1)] for b in range(B)])
    return idx, flags, moved


def backward_pass(latents, log_weights, locations, scale, uniforms):
    """The whole backward pass: latents T x [B,K,...], log_weights T x [B,K], locations(t) -> the transition's location
    [B,K,...] of step t's stored particles for time t+1, scale as above, uniforms T x [B,M] (block t draws step t).
    Returns (trajectories T x [B,M,...], indices T x [B,M])."""
    T = len(latents)
    states, indices = [None] * T, [None] * T
    indices[-1], _, states[-1] = backward_sample(log_weights[-1], None, None, None, uniforms[-1], latents[-1])
    for t in range(T - 2, -1, -1):
        indices[t], _, states[t] = backward_sample(log_weights[t], locations(t), states[t + 1], scale, uniforms[t],
                                                   latents[t])
    return states, indices
