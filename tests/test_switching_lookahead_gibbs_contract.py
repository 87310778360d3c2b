"""CPU checks of look-ahead particle Gibbs on the regimes of a switching linear-Gaussian model: the NumPy contract of kernels
K48 and K49 (aesmc_amd/testing/switching_lookahead_gibbs.py) against the parts it is made of, the invariance of one sweep
under the exact joint law of the regime sequences — and three wrong samplers that the same check rejects —, the host logic of
`conditional_switching_filter(..., lookahead=True)` and `switching_particle_gibbs(..., lookahead=True)` on an oracle
provider, and the ABI's argument checks of the three new entries."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_lookahead_gibbs as lookahead
from aesmc_amd.testing import switching_missing as missing
from tests.test_switching_gibbs_contract import (CHAINS, GibbsOracle, assert_within_five_standard_errors, invariance_case,
                                                 sweep_case)
from tests.test_switching_smoother_contract import _block, _torch_model


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


def step_case(B, K, M, D, Dy, steps, seed=0):
    """(model, log_Pi, particles, y, u, regime_next [B], F [B,TD], lam [B,D]) of one look-ahead conditional resampling step:
    the stored particles and the observation of `example_backward_step`, (F, lam) from `steps` information steps."""
    model, regime_next, info, y, particles, _ = contract.example_backward_step(B, K, 1, M, D, Dy, steps=steps, seed=seed)
    _, lam, _, F, flags, margin = contract.switching_information_step(model, regime_next, info, y)
    assert flags == 0 and margin > 1e-13
    u = np.random.default_rng([seed, B, K, M, D, Dy, steps, 48]).uniform(size=(B, K))
    return model, _log(model["Pi"]), particles, y, u, regime_next[:, 0].copy(), F[:, 0].copy(), lam[:, 0].copy()


# ---- 1. the contract against its parts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 2, 2, 2, 1), (3, 7, 2, 2, 3), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_the_index_function_is_the_lookahead_and_two_conditional_resamplings(shape):
    B, K, M, D, Dy = shape
    model, log_Pi, particles, y, u, regime_next, F, lam = step_case(B, K, M, D, Dy, 2)
    idx, log_w, cdf, flags, margins, score_bound, bounds = lookahead.lookahead_conditional_ancestor_index(
        model, log_Pi, particles, y, u, regime_next, F, lam)
    assert flags == 0 and idx.dtype == np.int64 and idx.shape == (B, K) and margins.shape == (B, K)
    want_w, want_cdf, bits = contract.switching_lookahead(model, log_Pi, particles, y)
    assert bits == 0 and np.array_equal(log_w, want_w) and np.array_equal(cdf, want_cdf)
    for got, want in zip(bounds, contract.switching_lookahead_bound(model, log_Pi, particles, y)):
        assert np.array_equal(got, want)
    free, bits, free_margins, _ = contract.switching_conditional_ancestor_index(log_w, u, None, None, None, None, None)
    assert bits == 0 and np.array_equal(idx[:, :K - 1], free[:, :K - 1])
    assert np.array_equal(margins[:, :K - 1], free_margins[:, :K - 1])
    # the pinned slot: K37's over a log-weight of exactly zero — NOT over the first-stage weights
    pinned, bits, pinned_margins, bound = contract.switching_conditional_ancestor_index(np.zeros((B, K)), u, log_Pi, regime_next,
                                                                                        F, lam, particles)
    assert bits == 0 and np.array_equal(idx[:, K - 1], pinned[:, K - 1]) and np.array_equal(score_bound, bound)
    assert np.array_equal(margins[:, K - 1], pinned_margins[:, K - 1])
    # without ancestor sampling the pinned slot keeps its ancestor
    plain = lookahead.lookahead_conditional_ancestor_index(model, log_Pi, particles, y, u, regime_next, None, None)
    assert plain[3] == 0 and (plain[0][:, K - 1] == K - 1).all() and np.array_equal(plain[0][:, :K - 1], idx[:, :K - 1])
    assert np.array_equal(plain[1], log_w) and (plain[5] == 0).all()


def test_the_pinned_scores_differ_from_the_weighted_ones_on_these_inputs():
    """The mutant below is not vacuous: with the first-stage weights in the pinned scores some ancestors change."""
    B, K, M, D, Dy = 64, 9, 3, 2, 2
    model, log_Pi, particles, y, u, regime_next, F, lam = step_case(B, K, M, D, Dy, 2)
    idx, log_w = lookahead.lookahead_conditional_ancestor_index(model, log_Pi, particles, y, u, regime_next, F, lam)[:2]
    weighted = contract.switching_conditional_ancestor_index(log_w, u, log_Pi, regime_next, F, lam, particles)[0]
    assert (weighted[:, K - 1] != idx[:, K - 1]).any() and np.array_equal(weighted[:, :K - 1], idx[:, :K - 1])


def test_bad_rows():
    B, K, M, D, Dy = 4, 9, 3, 2, 2
    model, log_Pi, particles, y, u, regime_next, F, lam = step_case(B, K, M, D, Dy, 2)
    run = lambda **kw: lookahead.lookahead_conditional_ancestor_index(
        kw.get("model", model), kw.get("log_Pi", log_Pi), kw.get("particles", particles), y, u,
        kw.get("regime_next", regime_next), F, lam)
    clean = run()
    assert clean[3] == 0
    # a stored regime outside [0, M): a NaN first-stage weight, every slot of the row
    regime = particles[0].copy()
    regime[1, 4] = M
    got = run(particles=(regime, particles[1], particles[2]))
    assert got[3] & contract.FLAG_INDEX_OUT_OF_RANGE and got[3] & contract.FLAG_NAN_LOG_WEIGHT
    assert (got[0][1] == K).all() and np.isnan(got[1][1, 4]) and np.isnan(got[2][1, 4]).all()
    assert np.array_equal(np.delete(got[0], 1, 0), np.delete(clean[0], 1, 0)) and np.isinf(got[4][1]).all()
    # a pinned regime outside [0, M): only slot K-1 of that row
    outside = regime_next.copy()
    outside[2] = -1
    got = run(regime_next=outside)
    assert got[3] == contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT and got[0][2, K - 1] == K
    assert np.array_equal(got[0][:, :K - 1], clean[0][:, :K - 1]) and np.array_equal(np.delete(got[0], 2, 0), np.delete(clean[0], 2, 0))
    # a zero column of Pi into s'_t: the first-stage weights stay finite (the other columns), only slot K-1 fails
    blocked = np.array(model["Pi"])
    blocked[:, regime_next[0]] = 0.0
    blocked /= blocked.sum(axis=1, keepdims=True)
    got = run(log_Pi=_log(blocked))
    hit = regime_next == regime_next[0]
    assert got[3] == contract.FLAG_DEGENERATE_ROW and (got[0][hit, K - 1] == K).all() and (got[0][:, :K - 1] < K).all()
    assert (got[0][~hit, K - 1] < K).all()
    # a pivot that is not positive under a regime of positive prior: NaN first-stage weights
    broken = dict(model, r=np.zeros_like(model["r"]), q=np.zeros_like(model["q"]))
    flat = (particles[0], particles[1], np.zeros_like(particles[2]))
    got = run(model=broken, particles=flat)
    assert got[3] & contract.FLAG_NAN_LOG_WEIGHT and (got[0] == K).all() and np.isnan(got[1]).all()


def test_a_row_that_measured_nothing_has_equal_weights_and_draws_from_the_transition():
    B, K, M, D, Dy = 3, 7, 3, 2, 3
    model, log_Pi, particles, y, u, regime_next, F, lam = step_case(B, K, M, D, Dy, 1)
    observed = np.ones((B, Dy), dtype=bool)
    observed[1] = False
    observed[2, 0] = False
    y = y.copy()
    y[1] = np.nan      # (never read)
    idx, log_w, cdf, flags, margins, _, _ = lookahead.lookahead_conditional_ancestor_index(
        model, log_Pi, particles, y, u, regime_next, F, lam, observed=observed)
    assert flags == 0
    np.testing.assert_allclose(log_w[1], 0.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(cdf[1], np.cumsum(model["Pi"], axis=1)[particles[0][1]], rtol=0, atol=1e-15)
    want_w, want_cdf, _ = missing.switching_lookahead(model, log_Pi, particles, y, observed)
    assert np.array_equal(log_w, want_w) and np.array_equal(cdf, want_cdf)
    # equal weights: slot k's ancestor is floor(u K), up to the rounding of the running sum
    assert (np.abs(idx[1, :K - 1] - np.floor(u[1, :K - 1] * K)) <= 1).all()
    # the step draws the regime of the free slots from those rows, the pinned slot takes the reference's
    regime_u = np.random.default_rng(5).uniform(size=(B, K))
    regime, mean, cov, ell, flags = lookahead.switching_kalman_conditional_draw(
        model, particles, np.minimum(idx, K - 1), regime_u, cdf, regime_next, y, observed=observed)
    assert flags == 0 and np.array_equal(regime[:, K - 1], regime_next) and (ell[1] == 0).all()
    rows = cdf[np.arange(B)[:, None], np.minimum(idx, K - 1)]
    assert np.array_equal(regime[:, :K - 1], (rows[:, :K - 1, :M - 1] <= regime_u[:, :K - 1, None]).sum(axis=2))
    free = missing.switching_kalman_draw(model, particles, np.minimum(idx, K - 1), regime_u, cdf, y, observed)
    pin = missing.switching_kalman_conditional_step(model, particles, np.minimum(idx, K - 1), regime_u, regime_next, y, observed)
    for part, a, b in zip((regime, mean, cov, ell), free[:4], pin[:4]):
        assert np.array_equal(part[:, :K - 1], a[:, :K - 1]) and np.array_equal(part[:, K - 1], b[:, K - 1])


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_one_regime_returns_the_reference_and_the_kalman_filters_means(ancestor_sampling):
    T, B, K = 4, 2, 5
    ops, model, observations, reference, uniforms, regime_u = sweep_case(T, B, K, 1, 3, 2, 4)
    ys = [y.numpy() for y in observations]
    out = lookahead.lookahead_conditional_switching_pass(ys, ops, K, reference, uniforms, regime_u,
                                                         ancestor_sampling=ancestor_sampling)
    assert out["flags"] == 0 and all((p == 0).all() for p in out["path"])
    state = None
    for t in range(T):      # the Kalman filter: K31 with one regime, no resampling (every particle is the same)
        regime, mean, cov, log_w, _ = contract.switching_kalman_step(ops, state, None, regime_u[t], ys[t])
        state = (regime, mean, cov)
        np.testing.assert_allclose(out["means"][t], mean, rtol=0, atol=1e-12)
        np.testing.assert_allclose(out["covariances"][t], cov, rtol=0, atol=1e-12)
        np.testing.assert_allclose(out["first_stage_log_weights"][t], log_w, rtol=0, atol=1e-12)      # p(y_t | y_{0:t-1})
        assert (out["log_weights"][t] == 0).all()


# ---- 2. invariance, and three wrong samplers -----------------------------------------------------------------------------------------
def _sweep(observations, ops, K, reference, uniforms, regime_u, ancestor_sampling, variant=None):
    """The look-ahead sweep assembled from the contract's pieces, with one of three mistakes on request:
    "weighted pin": the pinned slot's ancestor score carries the first-stage weight; "blind free": the free slots resample on
    equal weights; "weighted end": the final draw is weighted by the step's likelihood."""
    T, B = len(observations), observations[0].shape[0]
    log_pi0, log_Pi = _log(ops["pi0"]), _log(ops["Pi"])
    information = [None] * (T - 1)
    if ancestor_sampling:
        information = contract.switching_information_pass(ops, [r[:, None] for r in reference], observations)["information"]
    state, idx, regimes, ancestors = None, None, [], []
    for t in range(T):
        if t == 0:
            _, cdf, _ = contract.switching_lookahead(ops, log_pi0, None, observations[0], K)
        else:
            log_v, cdf, _ = contract.switching_lookahead(ops, log_Pi, state, observations[t])
            free = np.zeros_like(log_v) if variant == "blind free" else log_v
            idx = contract.switching_conditional_ancestor_index(free, uniforms[t - 1], None, None, None, None, None)[0]
            if ancestor_sampling:
                F, lam = information[t - 1][3][:, 0, :], information[t - 1][1][:, 0, :]
                carried = log_v if variant == "weighted pin" else np.zeros_like(log_v)
                idx[:, K - 1] = contract.switching_conditional_ancestor_index(carried, uniforms[t - 1], log_Pi, reference[t], F,
                                                                              lam, state)[0][:, K - 1]
            ancestors.append(idx)
        regime, mean, cov, ell, flags = lookahead.switching_kalman_conditional_draw(ops, state, idx, regime_u[t], cdf,
                                                                                    reference[t], observations[t])
        assert flags == 0
        state = (regime, mean, cov)
        regimes.append(regime)
    final = ell if variant == "weighted end" else np.zeros((B, K))
    at = contract.categorical_draw(final, uniforms[T - 1].reshape(B))[0]
    path, rows = [None] * T, np.arange(B)
    for t in range(T - 1, -1, -1):
        path[t] = regimes[t][rows, at]
        if t:
            at = ancestors[t - 1][rows, at]
    return np.stack(path)


@pytest.fixture(scope="module")
def invariance_inputs():
    """{ancestor_sampling: (observations, ops, reference, uniforms, regime_u, sequences, probabilities)}: 8192 references
    from the exact joint law and the uniforms of one sweep with K = 3, drawn in tests/test_switching_gibbs_contract.py's
    order; computed once."""
    ops, series, sequences, probabilities = invariance_case()
    T, K, out = len(series), 3, {}
    for ancestor_sampling in (True, False):
        rng = np.random.default_rng(483 + int(ancestor_sampling))
        start = sequences[rng.choice(len(sequences), size=CHAINS, p=probabilities)]
        reference = [start[:, t].astype(np.int32) for t in range(T)]
        observations = [np.broadcast_to(y, (CHAINS, 1)).copy() for y in series]
        uniforms = [rng.uniform(size=(CHAINS, K)) for _ in range(T - 1)] + [rng.uniform(size=(CHAINS, 1))]
        regime_u = [rng.uniform(size=(CHAINS, K)) for _ in range(T)]
        out[ancestor_sampling] = (observations, ops, reference, uniforms, regime_u, sequences, probabilities)
    return out


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_one_lookahead_sweep_leaves_the_exact_posterior_invariant(invariance_inputs, ancestor_sampling):
    """8192 independent references from the exact joint law, ONE look-ahead sweep each with K = 3: the new paths have that
    law.  The sweep assembled from the pieces in this file (the mutants' base) is the contract's pass, path for path."""
    observations, ops, reference, uniforms, regime_u, sequences, probabilities = invariance_inputs[ancestor_sampling]
    out = lookahead.lookahead_conditional_switching_pass(observations, ops, 3, reference, uniforms, regime_u,
                                                         ancestor_sampling=ancestor_sampling)
    assert out["flags"] == 0
    paths = np.stack(out["path"])
    assert (paths != np.stack(reference)).any()
    assert np.array_equal(paths, _sweep(observations, ops, 3, reference, uniforms, regime_u, ancestor_sampling))
    assert_within_five_standard_errors(paths, sequences, probabilities,
                                       "look-ahead, " + ("ancestor sampling" if ancestor_sampling else "plain"))


@pytest.mark.parametrize("variant,ancestor_sampling", [("weighted pin", True), ("blind free", True), ("blind free", False),
                                                       ("weighted end", True), ("weighted end", False)])
def test_the_check_rejects_three_wrong_samplers(invariance_inputs, variant, ancestor_sampling):
    """The same inputs, the same check, one mistake each: the check FAILS.  (This is the test that the check can fail.)"""
    observations, ops, reference, uniforms, regime_u, sequences, probabilities = invariance_inputs[ancestor_sampling]
    paths = _sweep(observations, ops, 3, reference, uniforms, regime_u, ancestor_sampling, variant=variant)
    with pytest.raises(AssertionError):
        assert_within_five_standard_errors(paths, sequences, probabilities, variant)


# ---- 3. the host logic on the oracle provider ------------------------------------------------------------------------------------------
class LookaheadOracle(GibbsOracle):
    """`GibbsOracle` plus K48 and K49 from their contract; `cap`: the fused launch's largest K (beyond it: composed)."""
    cap = 64

    def switching_lookahead(self, model, log_prior, state, observation, num_particles=None):
        self.calls.append("lookahead0" if state is None else "lookahead")
        return super().switching_lookahead(model, log_prior, state, observation, num_particles)

    def switching_lookahead_conditional_max_particles(self, num_regimes, latent_dim, observation_dim):
        return self.cap

    def switching_lookahead_conditional_ancestor_index(self, model, log_Pi, state, observation, u, regime_next, factor, lam,
                                                       fused=None):
        from aesmc_amd import _kernels
        if not (u.size(1) <= self.cap if fused is None else fused):
            return _kernels.compose_switching_lookahead_conditional(self, model, log_Pi, state, observation, u, regime_next,
                                                                    factor, lam)
        self.calls.append("fused" if factor is not None else "fused plain")
        ops, parts = self._numpy(model, state)
        idx, log_w, cdf, flags = lookahead.lookahead_conditional_ancestor_index(
            ops, log_Pi.numpy(), parts, observation.numpy(), u.numpy(), regime_next.numpy(),
            None if factor is None else factor.numpy(), None if lam is None else lam.numpy())[:4]
        self._flags |= flags
        return torch.from_numpy(idx), torch.from_numpy(log_w), torch.from_numpy(cdf)

    def switching_kalman_conditional_draw(self, model, state, index, uniforms, cdf, pinned_regime, observation):
        self.calls.append("draw step")
        ops, parts = self._numpy(model, state)
        regime, mean, cov, ell, flags = lookahead.switching_kalman_conditional_draw(
            ops, parts, None if index is None else index.numpy(), uniforms.numpy(), cdf.numpy(), pinned_regime.numpy(),
            observation.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(ell)


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = LookaheadOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _tensors(blocks):
    return [torch.from_numpy(block) for block in blocks]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_replayed_uniforms_give_the_contracts_pass_in_the_documented_launch_order(backend, ancestor_sampling, fused):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 5, 3, 9, 3, 2, 2
    backend.cap = 64 if fused else 8      # (the provider's cap decides between the one launch and the composition)
    ops, model, observations, reference, uniforms, regime_u = sweep_case(T, B, K, M, D, Dy, 5)
    path, particles = rao_blackwell.conditional_switching_filter(
        observations, model, K, _tensors(reference), ancestor_sampling=ancestor_sampling, uniforms=_tensors(uniforms),
        regime_uniforms=_tensors(regime_u), return_particles=True, lookahead=True)
    assert backend.reads == 1                                                                       # flags: read once
    backward = ["information0"] + ["information"] * (T - 2) if ancestor_sampling else []
    if fused:
        resample = ["fused" if ancestor_sampling else "fused plain"]
    else:
        resample = ["lookahead", "resample plain"] + (["resample"] if ancestor_sampling else [])
    assert backend.calls == backward + ["lookahead0", "draw step"] + (resample + ["draw step"]) * (T - 1) + \
        ["draw {}x1".format(B)]
    assert (backend.weights[-1] == 0).all()                                                         # the final draw: equal weights
    want = lookahead.lookahead_conditional_switching_pass([y.numpy() for y in observations], ops, K, reference, uniforms,
                                                          regime_u, ancestor_sampling=ancestor_sampling)
    assert want["flags"] == 0 and len(path) == T
    assert sorted(particles) == ["ancestral_indices", "covariances", "first_stage_log_weights", "indices", "log_weights",
                                 "means", "regimes"]
    for t in range(T):
        assert path[t].dtype == torch.int32 and path[t].shape == (B,) and np.array_equal(path[t].numpy(), want["path"][t])
        assert np.array_equal(particles["regimes"][t].numpy(), want["regimes"][t])
        assert np.array_equal(particles["regimes"][t][:, K - 1].numpy(), reference[t])              # the reference sits in slot K-1
        assert np.array_equal(particles["means"][t].numpy(), want["means"][t])
        assert (particles["log_weights"][t] == 0).all() and particles["log_weights"][t].shape == (B, K)
        assert np.array_equal(particles["first_stage_log_weights"][t].numpy(), want["first_stage_log_weights"][t])
        assert np.array_equal(particles["indices"][t].numpy(), want["indices"][t])
    for got, expected in zip(particles["ancestral_indices"], want["ancestral_indices"]):
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), expected)
        assert ancestor_sampling or (got[:, K - 1] == K - 1).all()
    if ancestor_sampling:      # the reference's ancestry is broken somewhere (a property of these seeds)
        assert any((a[:, K - 1] != K - 1).any() for a in want["ancestral_indices"])


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_without_lookahead_the_calls_are_the_parents(backend, ancestor_sampling):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 5, 3, 9, 3, 2, 2
    ops, model, observations, reference, uniforms, regime_u = sweep_case(T, B, K, M, D, Dy, 5)
    args = dict(ancestor_sampling=ancestor_sampling, uniforms=_tensors(uniforms), regime_uniforms=_tensors(regime_u),
                return_particles=True)
    path, particles = rao_blackwell.conditional_switching_filter(observations, model, K, _tensors(reference), lookahead=False,
                                                                 **args)
    backward = ["information0"] + ["information"] * (T - 2) if ancestor_sampling else []
    resample = "resample" if ancestor_sampling else "resample plain"
    assert backend.calls == backward + ["step"] + [resample, "step"] * (T - 1) + ["draw {}x1".format(B)]
    assert sorted(particles) == ["ancestral_indices", "covariances", "indices", "log_weights", "means", "regimes"]
    want = contract.conditional_switching_pass([y.numpy() for y in observations], ops, K, reference, uniforms, regime_u,
                                               ancestor_sampling=ancestor_sampling)
    assert all(np.array_equal(path[t].numpy(), want["path"][t]) for t in range(T))
    again = rao_blackwell.conditional_switching_filter(observations, model, K, _tensors(reference), **args)[0]
    assert all(torch.equal(a, b) for a, b in zip(path, again))


def test_fresh_uniforms_are_drawn_in_the_documented_order(backend):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 4, 2, 6, 2, 2, 1
    ops, model, observations, reference, _, _ = sweep_case(T, B, K, M, D, Dy, 2)
    reference = _tensors(reference)
    torch.manual_seed(21)
    fresh, particles = rao_blackwell.conditional_switching_filter(observations, model, K, reference, return_particles=True,
                                                                  lookahead=True)
    torch.manual_seed(21)
    draw = lambda columns: torch.rand((B, columns), dtype=torch.float64)
    regime_u, uniforms = [draw(K)], []
    for _ in range(1, T):
        uniforms.append(draw(K))
        regime_u.append(draw(K))
    uniforms.append(draw(1))
    replay, again = rao_blackwell.conditional_switching_filter(observations, model, K, reference, uniforms=uniforms,
                                                               regime_uniforms=regime_u, return_particles=True, lookahead=True)
    assert all(torch.equal(a, b) for a, b in zip(fresh, replay))
    assert all(torch.equal(a, b) for a, b in zip(particles["ancestral_indices"], again["ancestral_indices"]))
    assert all(torch.equal(a, b) for a, b in zip(particles["regimes"], again["regimes"]))


def test_one_particle_returns_the_reference_and_one_timestep_has_no_resampling(backend):
    from aesmc_amd import rao_blackwell
    T, B, M = 4, 3, 3
    ops, model, observations, reference, _, _ = sweep_case(T, B, 1, M, 2, 2, 3)
    reference = _tensors(reference)
    for ancestor_sampling in (True, False):
        path = rao_blackwell.conditional_switching_filter(observations, model, 1, reference, ancestor_sampling=ancestor_sampling,
                                                          lookahead=True)
        assert all(torch.equal(a, b) for a, b in zip(path, reference))
    backend.calls.clear()
    path, particles = rao_blackwell.conditional_switching_filter(observations[:1], model, 5, reference[:1], lookahead=True,
                                                                 return_particles=True)
    assert backend.calls == ["lookahead0", "draw step", "draw {}x1".format(B)] and len(path) == 1 and path[0].shape == (B,)
    assert len(particles["first_stage_log_weights"]) == 1 and particles["ancestral_indices"] == []


def test_refusals(backend):
    from aesmc_amd import distributed, rao_blackwell
    T, B, K = 3, 2, 4
    ops, model, observations, reference, uniforms, regime_u = sweep_case(T, B, K, 2, 2, 1, 6)
    reference, uniforms, regime_u = _tensors(reference), _tensors(uniforms), _tensors(regime_u)
    run = lambda **kw: rao_blackwell.conditional_switching_filter(
        kw.pop("observations", observations), kw.pop("model", model), kw.pop("num_particles", K),
        kw.pop("reference", reference), lookahead=True, **kw)
    with pytest.raises(ValueError, match="at least one timestep"):
        run(observations=[], reference=[])
    with pytest.raises(ValueError, match="num_particles must be at least 1"):
        run(num_particles=0)
    with pytest.raises(ValueError, match=r"reference must hold one tensor per timestep \(3\), got 2"):
        run(reference=reference[:2])
    with pytest.raises(ValueError, match=r"reference\[1\] must be \(2,\) int32"):
        run(reference=[reference[0], reference[1].to(torch.int64), reference[2]])
    with pytest.raises(ValueError, match="uniforms must hold one block per timestep"):
        run(uniforms=uniforms[:2])
    with pytest.raises(ValueError, match=r"uniforms\[2\] must be \(2, 1\) float64"):
        run(uniforms=uniforms[:2] + [torch.rand(B, K, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"uniforms\[0\] must be \(2, 4\) float64"):
        run(uniforms=[torch.rand(B, K)] + uniforms[1:])
    with pytest.raises(ValueError, match=r"regime_uniforms\[1\] must be \(2, 4\) float64"):
        run(regime_uniforms=[regime_u[0], torch.rand(B, K + 1, dtype=torch.float64), regime_u[2]])
    with pytest.raises(ValueError, match="observations must be"):
        run(observations=[torch.zeros(B, 3, dtype=torch.float64)] * T)
    with pytest.raises(NotImplementedError, match="num_particles = 8193.*covered: "):      # K37's cap, as without look-ahead
        run(num_particles=8193)
    wide = _torch_model(contract.example_model(2, 5, 1, seed=1))
    with pytest.raises(NotImplementedError, match="num_particles = 4097 with a latent of 5 values"):
        rao_blackwell.conditional_switching_filter(wide.simulate(T, B, seed=1), wide, 4097, reference, lookahead=True)
    with distributed.shard_scope(4, 0, 2), pytest.raises(NotImplementedError, match="shard_scope"):
        run()
    with distributed.shard_scope(4, 0, 2):      # a full replay is taken
        assert len(run(uniforms=uniforms, regime_uniforms=regime_u)) == T


def test_an_impossible_reference_raises_and_an_exception_discards_pending_flags(backend):
    from aesmc_amd import rao_blackwell
    from tests.test_switching_smoother_contract import MODEL_KEYS
    T, B, K = 3, 2, 4
    ops = contract.example_model(2, 2, 1, seed=6)
    ops = contract.operands(*[dict(ops, Pi=np.array([[1.0, 0.0], [1.0, 0.0]]), pi0=np.array([1.0, 0.0]))[name]
                              for name in MODEL_KEYS])
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=1)
    reference = [torch.zeros(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match="no finite maximum"):
        rao_blackwell.conditional_switching_filter(observations, model, K, reference, lookahead=True)
    assert backend.read_flags(None) == 0
    bad = [torch.rand(B, K, dtype=torch.float64), torch.rand(B, K, dtype=torch.float64), torch.rand(B, 2, dtype=torch.float64)]
    with pytest.raises(ValueError, match=r"uniforms\[2\]"):      # raised after the loop: the flags of step 1 are pending
        rao_blackwell.conditional_switching_filter(observations, model, K, reference, uniforms=bad, lookahead=True)
    assert backend.read_flags(None) == 0


def test_a_nan_first_stage_weight_of_step_zero_raises_after_the_one_flag_read(backend):
    """Step 0's first-stage weights meet no resampling launch: with s0 = 0 and r = 0 the innovation covariance of step 0 is
    zero, no pivot is positive, the weights are NaN and nothing flags them; the sweep raises FloatingPointError itself."""
    from aesmc_amd import rao_blackwell
    from tests.test_switching_smoother_contract import MODEL_KEYS
    B, K = 2, 4
    ops = contract.example_model(2, 2, 1, seed=6)
    ops = contract.operands(*[dict(ops, s0=np.zeros(2), r=np.zeros((2, 1)))[name] for name in MODEL_KEYS])
    model = _torch_model(ops)
    observations = [torch.zeros(B, 1, dtype=torch.float64)]
    reference = [torch.zeros(B, dtype=torch.int32)]
    with pytest.raises(FloatingPointError, match="log_weight contains nan"):
        rao_blackwell.conditional_switching_filter(observations, model, K, reference, lookahead=True)
    assert backend.reads == 1 and backend.read_flags(None) == 0
    assert backend.calls == ["lookahead0", "draw step", "draw {}x1".format(B)]


def test_particle_gibbs_chains_lookahead_sweeps(backend):
    from aesmc_amd import rao_blackwell
    T, B, K, M = 4, 3, 5, 3
    ops, model, observations, reference, _, _ = sweep_case(T, B, K, M, 2, 2, 8)
    torch.manual_seed(5)
    out = rao_blackwell.switching_particle_gibbs(observations, model, K, 6, reference=_tensors(reference), burn_in=2,
                                                 lookahead=True)
    assert sorted(out) == ["regimes", "smoothed_regime_probabilities"] and len(out["regimes"]) == T
    assert all(r.shape == (B, 4) and r.dtype == torch.int32 for r in out["regimes"])
    assert "step" not in backend.calls and backend.calls.count("draw step") == 6 * T
    torch.manual_seed(5)
    path = _tensors(reference)
    for sweep in range(6):
        path = rao_blackwell.conditional_switching_filter(observations, model, K, path, lookahead=True)
        if sweep >= 2:
            assert all(torch.equal(out["regimes"][t][:, sweep - 2], path[t]) for t in range(T))
    # without a reference the first path is one trajectory of the look-ahead smoother
    backend.calls.clear()
    np.random.seed(5)
    out = rao_blackwell.switching_particle_gibbs(observations, model, K, 1, lookahead=True)
    first = backend.calls.index("draw step")
    assert backend.calls[:first].count("lookahead0") == 2 and "scores" in backend.calls[:first]      # the smoother's, the sweep's
    assert "step" not in backend.calls and out["regimes"][0].shape == (B, 1)


# ---- 4. the library built here ----------------------------------------------------------------------------------------------------------
def test_the_cap_function():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    cap = lib.aesmc_switching_lookahead_conditional_max_particles
    pad = lambda n: 2 if n <= 2 else 4 if n <= 4 else 8

    def formula(M, D, Dy):
        P, Q = pad(D), pad(Dy)
        T = P * (P + 1) // 2
        fixed = T + P + 30 + M * M + M * (P * P + 2 * P + Q * P + 2 * Q) + (256 * T if P == 8 else 0) + 256 * M
        return min(lib.aesmc_switching_conditional_max_particles(D), (160 * 1024 // 8 - fixed) // 2)

    for M in (1, 2, 4, 16):
        for D in (1, 2, 3, 4, 5, 8):
            for Dy in (1, 2, 3, 4, 5, 8):
                assert cap(M, D, Dy) == formula(M, D, Dy) > 64, (M, D, Dy)
                assert cap(M, D, Dy) <= lib.aesmc_switching_conditional_max_particles(D)
    assert cap(1, 1, 1) == 8192 and cap(4, 4, 4) == 8192 and cap(4, 8, 8) == 4096 and cap(16, 8, 8) < 4096
    for M, D, Dy in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (17, 1, 1), (1, 9, 1), (1, 1, 9), (-1, 2, 2)):
        assert cap(M, D, Dy) == 0, (M, D, Dy)


@pytest.mark.parametrize("masked", [False, True])
def test_the_abi_of_the_fused_resampling_rejects_bad_arguments_before_any_launch(masked):
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    block = lambda **kw: _block(_lib, **kw)
    cap = lib.aesmc_switching_lookahead_conditional_max_particles

    def call(model="default", log_Pi=128, regime=132, mean=136, cov=144, y=152, observed=161, u=168, regime_next=180, factor=184,
             lam=192, out=256, log_weight=264, cdf=272, flags=64, B=1, K=4, dtype=1):
        model = block() if model == "default" else model
        pointer = None if model is None else ctypes.byref(model)
        if masked:
            return lib.aesmc_switching_masked_lookahead_conditional_ancestor_index(
                dtype, pointer, log_Pi, regime, mean, cov, y, observed, u, regime_next, factor, lam, out, log_weight, cdf, flags,
                B, K, None)
        return lib.aesmc_switching_lookahead_conditional_ancestor_index(
            dtype, pointer, log_Pi, regime, mean, cov, y, u, regime_next, factor, lam, out, log_weight, cdf, flags, B, K, None)

    for name in ("model", "log_Pi", "regime", "mean", "cov", "y", "u", "out", "log_weight", "cdf"):
        assert call(**{name: None}) == 1, name
    if masked:
        assert call(observed=None) == 1 and call(out=160, observed=160) == 1 and call(observed=161, B=0) == 0      # bytes
    assert call(factor=None) == 1 and call(lam=None) == 1 and call(regime_next=None) == 1           # they come together
    assert call(factor=None, lam=None, regime_next=None, B=0) == 0                                  # no ancestor sampling
    for name in ("A", "b", "q", "C", "d", "r"):
        assert call(model=block(**{name: None})) == 1 and call(model=block(**{name: 68})) == 1, name
    assert call(model=block(cdf0=None, cdf=None, m0=None, s0=None), B=0) == 0                       # (not read)
    assert call(flags=None, B=0) == 0
    for name, value in (("log_Pi", 132), ("regime", 134), ("mean", 140), ("cov", 148), ("y", 156), ("u", 172),
                        ("regime_next", 182), ("factor", 188), ("lam", 196), ("out", 260), ("log_weight", 268), ("cdf", 276),
                        ("flags", 66)):
        assert call(**{name: value}) == 1, name
    assert call(y=154, dtype=0) == 1 and call(y=156, dtype=0, B=0) == 0 and call(dtype=7) == 1
    assert call(B=-1) == 1 and call(K=-1) == 1
    assert call(model=block(M=0)) == 1 and call(model=block(D=0)) == 1 and call(model=block(Dy=0)) == 1
    for value in (128, 136, 144, 152, 168, 184, 192):
        assert call(out=value) == 1, value                                                          # an output is an operand
    assert call(log_weight=136) == 1 and call(cdf=144) == 1 and call(cdf=264) == 1 and call(log_weight=256) == 1
    assert call(model=block(D=9)) == 2 and call(model=block(Dy=9)) == 2 and call(model=block(M=17)) == 2
    assert call(K=cap(2, 3, 2) + 1) == 2 and call(K=8193) == 2
    assert call(model=block(M=16, D=8, Dy=8), K=cap(16, 8, 8) + 1) == 2 and cap(16, 8, 8) + 1 <= 4096
    assert call(B=1 << 31) == 2 and call(B=1 << 20, K=1 << 12) == 2
    assert call(B=0) == 0 and call(K=0) == 0 and call(B=0, model=block(D=9)) == 0 and call(K=0, model=block(M=17)) == 0


def test_the_abi_of_the_conditional_draw_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    block = lambda **kw: _block(_lib, **kw)

    def step(model="default", regime_in=128, mean_in=136, cov_in=144, idx=152, uniforms=160, cdf=176, pinned=164, y=168,
             regime_out=256, mean_out=264, cov_out=272, log_weight=280, flags=64, B=1, K=4, dtype=1):
        model = block() if model == "default" else model
        return lib.aesmc_switching_kalman_conditional_draw(dtype, None if model is None else ctypes.byref(model), regime_in,
                                                           mean_in, cov_in, idx, uniforms, cdf, pinned, y, regime_out,
                                                           mean_out, cov_out, log_weight, flags, B, K, None)

    assert step(model=None) == 1 and step(uniforms=None) == 1 and step(y=None) == 1
    assert step(pinned=None) == 1 and step(cdf=None) == 1                                           # K38's and K33's operands
    assert step(regime_out=None) == 1 and step(mean_out=None) == 1 and step(cov_out=None) == 1 and step(log_weight=None) == 1
    for name in ("m0", "s0", "A", "b", "q", "C", "d", "r"):
        assert step(model=block(**{name: None})) == 1 and step(model=block(**{name: 68})) == 1, name
    assert step(model=block(cdf=None, cdf0=None), B=0) == 0                                         # the chain's rows are not read
    assert step(regime_in=None) == 1 and step(mean_in=None) == 1 and step(cov_in=None) == 1        # a state given in part
    assert step(regime_in=None, mean_in=None, cov_in=None, idx=None, B=0) == 0                     # the step-0 form
    assert step(B=-1) == 1 and step(K=-1) == 1 and step(dtype=7) == 1
    assert step(model=block(M=0)) == 1 and step(model=block(D=0)) == 1 and step(model=block(Dy=0)) == 1
    assert step(regime_in=130) == 1 and step(mean_in=140) == 1 and step(cov_in=148) == 1 and step(idx=156) == 1
    assert step(uniforms=164) == 1 and step(pinned=166) == 1 and step(cdf=180) == 1 and step(y=172) == 1 and step(flags=66) == 1
    assert step(regime_out=258) == 1 and step(mean_out=268) == 1 and step(cov_out=276) == 1 and step(log_weight=284) == 1
    assert step(regime_out=128) == 1 and step(mean_out=136) == 1 and step(cov_out=144) == 1        # aliasing
    assert step(pinned=256) == 1 and step(cdf=264) == 1 and step(cdf=272) == 1 and step(cdf=280) == 1
    assert step(model=block(D=9)) == 2 and step(model=block(Dy=9)) == 2 and step(model=block(M=17)) == 2
    assert step(B=1 << 16, K=1 << 16) == 2
    assert step(B=0) == 0 and step(K=0) == 0 and step(B=0, model=block(D=9)) == 0 and step(flags=None, B=0) == 0
    assert step(y=172, dtype=0, B=0) == 0                                                          # float32 rows
