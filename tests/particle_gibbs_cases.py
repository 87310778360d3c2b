"""Operands and the statistical problem the particle-Gibbs tests share (tests/test_particle_gibbs_contract.py on the CPU,
tests/test_gpu_particle_gibbs.py on the device)."""
import numpy as np

from aesmc_amd.testing import smoothing as smoothing_contract

BELOW_ONE = 1.0 - 2.0 ** -53
# the weight / score profiles of tests/test_gpu_backward_simulation.py
PROFILES = ("flat", "unit", "wide", "minus_inf_stretch", "tied", "dominant", "far")


def operands(profile, B, K, D, dtype, seed):
    """(log_w [B,K], u [B,K] float64, loc [B,K,D], target [B,D], scale [D]) as NumPy arrays of `dtype` for one profile; a
    few uniforms are 0 and a few 1 - 2^-53, among them one of each in the pinned slot's column."""
    rng = np.random.RandomState(seed)
    log_w = rng.randn(B, K) * {"flat": 0.0, "wide": 10.0}.get(profile, 1.0)
    loc, target = rng.randn(B, K, D), rng.randn(B, D)
    scale = 0.5 + rng.rand(D)
    if profile == "minus_inf_stretch":
        log_w[:, K // 3:K // 3 + max(1, K // 4)] = -np.inf
        log_w[:, 0] = 0.0          # (K == 1: keep a particle)
    elif profile == "tied":        # every particle at the same location, equal weights: every score tied
        loc[:] = loc[:, :1]
        log_w[:] = 0.0
    elif profile == "dominant":
        log_w[np.arange(B), rng.randint(K, size=B)] += 60.0
    elif profile == "far":         # the target far from every location: most of the pinned slot's w underflows to zero
        target += 400.0
    u = rng.rand(B, K)
    u[rng.randint(B, size=3), rng.randint(K, size=3)] = 0.0
    u[rng.randint(B, size=3), rng.randint(K, size=3)] = BELOW_ONE
    u[0, K - 1] = 0.0 if seed % 2 else BELOW_ONE
    u[B - 1, 0] = BELOW_ONE if seed % 2 else 0.0
    return log_w.astype(dtype), u, loc.astype(dtype), target.astype(dtype), scale.astype(dtype)


def composed(log_w, u, loc, target, scale):
    """The K21 contract used as the issue of K26 describes: slots 0 .. K-2 without a term at u[:, :K-1], slot K-1 with
    M = 1 at u[:, K-1:] (no term: K-1).  Returns (idx [B,K], flags)."""
    B, K = log_w.shape
    free, flags, _ = smoothing_contract.backward_sample(log_w, None, None, None, u[:, :K - 1])
    if loc is None:
        pinned, more = np.full((B, 1), K - 1, dtype=np.int64), 0
    else:
        pinned, more, _ = smoothing_contract.backward_sample(log_w, loc, target[:, None], scale, u[:, K - 1:])
    return np.concatenate([free, pinned], axis=1), flags | more


# ---- the statistical problem: the scalar random walk of test_smoothed_posterior_against_the_exact_smoother, its first
# 25 steps, B = 256 chains of K = 8 particles started 60 units away from the data, 40 sweeps of which 10 are discarded
M0, P0, Q, R = 0.0, 100.0, 25.0, 64.0
STEPS, CHAINS, PARTICLES, SWEEPS, BURN_IN, AWAY = 25, 256, 8, 40, 10, 60.0
# Bounds from the NumPy contract (aesmc_amd/testing/particle_gibbs.py) — see
# tests/test_particle_gibbs_contract.py::test_numpy_particle_gibbs_against_the_exact_smoother for the observed ranges
RMSE_BOUND, VARIANCE_BOUND, REPLACED_AT_LEAST = 0.25, 0.05, 0.5
PLAIN_REPLACED_AT_MOST, PLAIN_RMSE_AT_LEAST = 0.05, 0.5


def data():
    rng = np.random.RandomState(0)
    grid = np.linspace(0, 3 * np.pi, 100)
    return (40 * (np.sin(grid) + 0.2 * rng.randn(100)))[:STEPS]
