"""CPU checks of particle Gibbs with ancestor sampling: the NumPy contract of aesmc_conditional_ancestor_index
(aesmc_amd/testing/particle_gibbs.py) against the K21 contract it is defined by, its conventions for bad rows, the ABI's
argument checks, the restated sweep's properties, the host logic of `aesmc_amd.particle_gibbs` on a provider that adds the
two draws from the contracts to the suite's oracle provider, and the NumPy sampler against the exact smoother — where the
bounds of the device's statistical test come from."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import particle_gibbs as contract
from aesmc_amd.testing import smoothing as smoothing_contract
from tests import particle_gibbs_cases as cases
from tests.oracle_provider import OracleKernels


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D", [(1, 1, 1), (3, 7, 2), (2, 65, 3), (2, 300, 0)])
def test_contract_equals_the_backward_sample_contract(dtype, B, K, D):
    for number, profile in enumerate(cases.PROFILES):
        if D == 0 and profile in ("tied", "far"):
            continue      # (no transition term: nothing to tie or to move away)
        log_w, u, loc, target, scale = cases.operands(profile, B, K, max(D, 1), dtype, 100 * number + K % 89)
        if D == 0:
            loc = target = scale = None
        elif number % 2:
            scale = scale[:1]      # one value for the whole latent
        idx, flags = contract.conditional_ancestor_index(log_w, u, loc, target, scale)
        want, want_flags = cases.composed(log_w, u, loc, target, scale)
        assert flags == 0 and want_flags == 0 and idx.dtype == np.int64 and idx.shape == (B, K)
        np.testing.assert_array_equal(idx, want, err_msg=profile)
        assert (idx >= 0).all() and (idx < K).all()
        if D == 0:
            assert (idx[:, K - 1] == K - 1).all()
        if K == 1:
            assert (idx == 0).all()


def test_uniforms_at_the_ends():
    """u = 0 picks the first particle of positive weight, u = 1 - 2^-53 the last one (the clamp)."""
    log_w = np.array([[-np.inf, 0.0, -1.0, -3000.0, -np.inf]])
    loc, target, scale = np.zeros((1, 5, 1)), np.zeros((1, 1)), np.ones(1)
    idx, flags = contract.conditional_ancestor_index(log_w, np.zeros((1, 5)), loc, target, scale)
    assert flags == 0 and (idx == 1).all()
    idx, flags = contract.conditional_ancestor_index(log_w, np.full((1, 5), cases.BELOW_ONE), loc, target, scale)
    assert flags == 0 and (idx == 2).all()


def test_bad_rows_flag_and_leave_the_others_alone():
    B, K, D = 4, 30, 3
    log_w, u, loc, target, scale = cases.operands("unit", B, K, D, np.float32, 5)
    clean, flags = contract.conditional_ancestor_index(log_w, u, loc, target, scale)
    assert flags == 0 and (clean < K).all()

    def check(bad_log_w, bad_loc, bad_target, affected, bit):
        idx, flags = contract.conditional_ancestor_index(bad_log_w, u, bad_loc, bad_target, scale)
        want, want_flags = cases.composed(bad_log_w, u, bad_loc, bad_target, scale)
        assert flags == bit == want_flags
        assert (idx[affected] == K).all() and (idx[~affected] == clean[~affected]).all()
        np.testing.assert_array_equal(idx, want)

    row = lambda b: np.ones((B, K), dtype=bool) & (np.arange(B) == b)[:, None]
    slot = lambda b: row(b) & (np.arange(K) == K - 1)[None, :]
    nan_w = log_w.copy()
    nan_w[1, 7] = np.nan
    check(nan_w, loc, target, row(1), contract.FLAG_NAN_LOG_WEIGHT)
    dead = log_w.copy()
    dead[3] = -np.inf
    check(dead, loc, target, row(3), contract.FLAG_DEGENERATE_ROW)
    hot = log_w.copy()
    hot[0, 0] = np.inf
    check(hot, loc, target, row(0), contract.FLAG_DEGENERATE_ROW)
    nan_loc = loc.copy()
    nan_loc[2, 29, 1] = np.nan
    check(log_w, nan_loc, target, slot(2), contract.FLAG_NAN_LOG_WEIGHT)      # only the pinned slot
    nan_target = target.copy()
    nan_target[0, 2] = np.nan
    check(log_w, loc, nan_target, slot(0), contract.FLAG_NAN_LOG_WEIGHT)
    lost = loc.copy()
    lost[1] = np.inf                                                          # every score -inf: no finite maximum
    check(log_w, lost, target, slot(1), contract.FLAG_DEGENERATE_ROW)
    # without a transition term a bad row takes its pinned slot along
    idx, flags = contract.conditional_ancestor_index(dead, u)
    assert flags == contract.FLAG_DEGENERATE_ROW and (idx[3] == K).all() and (idx[:3, K - 1] == K - 1).all()


def test_the_abi_rejects_bad_arguments_before_any_launch():
    """NULL pointers and negative sizes give status 1, a transition term wider than 256 values or more than 8192
    particles status 2, an empty problem is a no-op — no GPU needed."""
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    view = _lib.View3(16, 4, 1, 1)
    ref = ctypes.byref(view)

    def call(log_w=16, u=16, loc=ref, target=ref, scale=16, scale_stride=0, idx=16, B=1, K=4, D=1, dtype=0):
        return lib.aesmc_conditional_ancestor_index(dtype, log_w, u, loc, target, scale, scale_stride, idx, None, B, K, D,
                                                    None)

    assert call(log_w=None) == 1 and call(u=None) == 1 and call(idx=None) == 1
    assert call(loc=None) == 1 and call(target=None) == 1 and call(scale=None) == 1
    assert call(loc=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1
    assert call(B=-1) == 1 and call(K=-1) == 1 and call(D=-1) == 1
    assert call(dtype=7) == 1 and call(scale_stride=2) == 1 and call(u=12) == 1 and call(idx=12) == 1
    assert call(D=257) == 2 and call(K=8193) == 2
    assert call(B=0) == 0 and call(K=0) == 0 and call(B=0, D=257) == 0
    assert call(loc=None, target=None, scale=None, D=0, B=0) == 0      # the D == 0 form takes NULL terms


# ---- the restated sweep ---------------------------------------------------------------------------------------------------
def _sweep_inputs(T, B, K, d, seed):
    rng = np.random.RandomState(seed)
    latents = [rng.randn(B, K, d) for _ in range(T)]
    log_weights = [rng.randn(B, K) for _ in range(T)]
    reference = [rng.randn(B, d) for _ in range(T)]
    uniforms = [rng.rand(B, K) for _ in range(T - 1)] + [rng.rand(B, 1)]
    return latents, log_weights, reference, uniforms


def test_conditional_pass_with_one_particle_returns_the_reference():
    latents, log_weights, reference, uniforms = _sweep_inputs(5, 3, 1, 2, 0)
    for ancestor_sampling in (True, False):
        path, stored, ancestral, indices = contract.conditional_pass(
            latents, log_weights, lambda t: 0.9 * stored_of(latents, reference, t), np.ones(1), reference, uniforms,
            ancestor_sampling)
        for t in range(5):
            assert np.array_equal(path[t].view(np.uint8), reference[t].view(np.uint8))
            assert (indices[t] == 0).all()


def stored_of(latents, reference, t):
    x = latents[t].copy()
    x[:, -1] = reference[t]
    return x


@pytest.mark.parametrize("ancestor_sampling", [False, True])
def test_conditional_pass_properties(ancestor_sampling):
    T, B, K, d = 6, 4, 9, 2
    latents, log_weights, reference, uniforms = _sweep_inputs(T, B, K, d, 1)
    path, stored, ancestral, indices = contract.conditional_pass(
        latents, log_weights, lambda t: 0.9 * stored_of(latents, reference, t), np.array([0.7, 1.1]), reference, uniforms,
        ancestor_sampling)
    rows = np.arange(B)
    for t in range(T):
        assert np.array_equal(stored[t][:, K - 1], reference[t])               # slot K-1 holds the reference
        assert np.array_equal(stored[t][:, :K - 1], latents[t][:, :K - 1])     # the free slots are the draws
        assert np.array_equal(path[t], stored[t][rows, indices[t]])
        if t < T - 1:
            assert np.array_equal(indices[t], ancestral[t][rows, indices[t + 1]])
            if not ancestor_sampling:
                assert (ancestral[t][:, K - 1] == K - 1).all()
            free, _, _ = smoothing_contract.backward_sample(log_weights[t], None, None, None, uniforms[t][:, :K - 1])
            assert np.array_equal(ancestral[t][:, :K - 1], free)
    if ancestor_sampling:      # the pinned slot's ancestor moves
        assert any((ancestral[t][:, K - 1] != K - 1).any() for t in range(T - 1))
    # a path that ends in the pinned slot and never leaves it is the reference
    if not ancestor_sampling:
        stuck = indices[T - 1] == K - 1
        for t in range(T):
            assert (indices[t][stuck] == K - 1).all()


# ---- the host logic on the oracle provider -----------------------------------------------------------------------------
class GibbsOracle(OracleKernels):
    """The suite's oracle provider plus the two draws from their NumPy contracts."""
    from aesmc_amd._kernels import HipKernels as _Hip
    conditional_ancestor_index_covers = staticmethod(_Hip.conditional_ancestor_index_covers)

    def __init__(self):
        super().__init__()
        self.calls = []

    def conditional_ancestor_index(self, log_w, u, loc=None, target=None, scale=None):
        n = lambda t: None if t is None else t.detach().numpy()
        self.calls.append(None if loc is None else tuple(scale.shape))
        idx, flags = contract.conditional_ancestor_index(n(log_w), n(u), n(loc), n(target), n(scale))
        self._flags |= flags
        return torch.from_numpy(idx)

    def backward_sample(self, log_w, loc, target, scale, u, payload=None):
        n = lambda t: None if t is None else t.detach().numpy()
        idx, flags, _ = smoothing_contract.backward_sample(n(log_w), n(loc), n(target), n(scale), n(u))
        self._flags |= flags
        return torch.from_numpy(idx), None


@pytest.fixture
def gibbs_backend():
    from aesmc_amd import _kernels
    provider = GibbsOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _problem(T=5, B=3, d=2, dtype=torch.float64, validate_args=None):
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(d, dtype=dtype, validate_args=validate_args).tune_proposal()
    observations = model.simulate(T, B, seed=1)
    gen = torch.Generator().manual_seed(5)
    reference = [torch.randn(B, d, dtype=dtype, generator=gen) for _ in range(T)]
    return model, observations, reference


def _uniforms(T, B, K, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(B, K if t < T - 1 else 1, dtype=torch.float64, generator=gen) for t in range(T)]


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_conditional_smc_equals_the_numpy_pass(gibbs_backend, ancestor_sampling):
    from aesmc_amd import particle_gibbs
    T, B, K, d = 5, 3, 12, 2
    model, observations, reference = _problem(T, B, d)
    uniforms = _uniforms(T, B, K)
    path, particles = particle_gibbs.conditional_smc(
        observations, model.initial, model.transition, model.emission, model.proposal, K, reference,
        ancestor_sampling=ancestor_sampling, uniforms=uniforms, return_particles=True)
    latents, log_weights = particles["latents"], particles["log_weights"]
    assert len(path) == T and len(latents) == T and len(log_weights) == T and len(particles["ancestral_indices"]) == T - 1
    with torch.no_grad():
        locations = [model.transition(previous_latents=latents[:t + 1], time=t + 1).loc.numpy() for t in range(T - 1)]
    want, stored, ancestral, indices = contract.conditional_pass(
        [x.numpy() for x in latents], [w.numpy() for w in log_weights], lambda t: locations[t],
        np.array([float(model.transition_scale)]), [x.numpy() for x in reference], [u.numpy() for u in uniforms],
        ancestor_sampling)
    for t in range(T):
        assert path[t].shape == (B, d) and not path[t].requires_grad and latents[t].shape == (B, K, d)
        assert torch.equal(latents[t][:, K - 1], reference[t])
        np.testing.assert_array_equal(path[t].numpy(), want[t])
        np.testing.assert_array_equal(particles["indices"][t].numpy(), indices[t])
        if t < T - 1:
            assert particles["ancestral_indices"][t].dtype == torch.int64
            np.testing.assert_array_equal(particles["ancestral_indices"][t].numpy(), ancestral[t])
    assert gibbs_backend.calls == ([(1,)] if ancestor_sampling else [None]) * (T - 1)
    # the weights are transition x emission / proposal under each slot's own ancestor, the pinned slot included
    t = 2
    previous = torch.gather(latents[t - 1], 1, particles["ancestral_indices"][t - 1].unsqueeze(-1).expand(B, K, d))
    with torch.no_grad():
        f = model.transition(previous_latents=[previous], time=t).log_prob(latents[t]).sum(-1)
        g = model.emission(latents=[latents[t]], time=t).log_prob(observations[t].unsqueeze(1)).sum(-1)
        q = model.proposal(previous_latents=[previous], time=t, observations=observations).log_prob(latents[t]).sum(-1)
    torch.testing.assert_close(log_weights[t], f + g - q, rtol=1e-12, atol=1e-12)


def test_conditional_smc_properties(gibbs_backend):
    from aesmc_amd import particle_gibbs
    model, observations, reference = _problem()
    run = lambda K, **kw: particle_gibbs.conditional_smc(observations, model.initial, model.transition, model.emission,
                                                         model.proposal, K, reference, **kw)
    for ancestor_sampling in (True, False):      # one particle: the reference, bit for bit
        path = run(1, ancestor_sampling=ancestor_sampling)
        assert all(torch.equal(a, b) for a, b in zip(path, reference))
    one = particle_gibbs.conditional_smc(observations[:1], model.initial, model.transition, model.emission, model.proposal,
                                         6, reference[:1])
    assert len(one) == 1 and one[0].shape == reference[0].shape
    np.random.seed(11)
    before = np.random.get_state()
    torch.manual_seed(3)
    first = run(8)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    torch.manual_seed(3)
    again = run(8)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    other = run(8)
    assert not all(torch.equal(a, b) for a, b in zip(first, other))


def test_refusals(gibbs_backend):
    from aesmc_amd import distributed, particle_gibbs, state
    T, B, K, d = 5, 3, 6, 2
    model, observations, reference = _problem(T, B, d)
    full = state.BatchShapeMode.FULLY_EXPANDED

    def run(transition=model.transition, K=K, reference=reference, **kw):
        return particle_gibbs.conditional_smc(observations, model.initial, transition, model.emission, model.proposal, K,
                                              reference, **kw)

    with pytest.raises(NotImplementedError, match="num_particles = 8193"):
        run(K=8193)
    assert gibbs_backend.calls == []
    with pytest.raises(ValueError, match="one tensor per timestep"):
        run(reference=reference[:-1])
    with pytest.raises(ValueError, match="reference"):
        run(reference=[x[:, :1] for x in reference])
    with pytest.raises(ValueError, match="reference"):
        run(reference=[x.float() for x in reference])
    with pytest.raises(NotImplementedError, match="dict"):
        run(reference=[{"x": x} for x in reference])
    assert gibbs_backend.calls == []

    def particle_scale(previous_latents=None, time=None, previous_observations=None):
        loc = previous_latents[-1] @ model.A.t()
        return state.set_batch_shape_mode(Normal(loc, torch.ones(B, K, d, dtype=torch.float64)), full)

    with pytest.raises(NotImplementedError, match="particle-dependent"):
        run(transition=particle_scale)
    path = run(transition=particle_scale, ancestor_sampling=False)      # plain conditional SMC takes any transition
    assert path[0].shape == (B, d)
    with distributed.shard_scope(2 * B, 0, 2):
        with pytest.raises(NotImplementedError, match="shard_scope"):
            run()
        run(uniforms=_uniforms(T, B, K))      # replayed blocks are fine
    with pytest.raises(ValueError, match="one block per timestep"):
        run(uniforms=_uniforms(T - 1, B, K))
    with pytest.raises(ValueError, match="float64"):
        run(uniforms=[u.float() for u in _uniforms(T, B, K)])
    with pytest.raises(ValueError, match="burn_in"):
        particle_gibbs.particle_gibbs(observations, model.initial, model.transition, model.emission, model.proposal, K, 3,
                                      reference=reference, burn_in=3)


def test_bad_rows_are_raised_once_at_the_end(gibbs_backend):
    from aesmc_amd import particle_gibbs, state
    model, observations, reference = _problem()

    def emission(latents=None, time=None, previous_observations=None):      # a NaN log-weight in row 1 of step 2
        loc = latents[-1] @ model.C.t()
        if time == 2:
            loc = loc.clone()
            loc[1, 0, 0] = float("nan")
        return state.set_batch_shape_mode(Normal(loc, model.emission_scale, validate_args=False),
                                          state.BatchShapeMode.FULLY_EXPANDED)

    with pytest.raises(FloatingPointError):
        particle_gibbs.conditional_smc(observations, model.initial, model.transition, emission, model.proposal, 6, reference)
    assert gibbs_backend.read_flags(None) == 0      # discarded with the exception
    particle_gibbs.conditional_smc(observations, model.initial, model.transition, model.emission, model.proposal, 6, reference)


def test_particle_gibbs_stacks_the_kept_sweeps(gibbs_backend):
    from aesmc_amd import particle_gibbs
    T, B, K, d = 4, 3, 6, 2
    model, observations, reference = _problem(T, B, d)
    torch.manual_seed(1)
    out = particle_gibbs.particle_gibbs(observations, model.initial, model.transition, model.emission, model.proposal, K,
                                        5, reference=reference, burn_in=2)
    assert len(out) == T and all(x.shape == (B, 3, d) for x in out)
    torch.manual_seed(1)
    path = reference
    for sweep in range(5):
        path = particle_gibbs.conditional_smc(observations, model.initial, model.transition, model.emission,
                                              model.proposal, K, path)
        if sweep >= 2:
            assert all(torch.equal(out[t][:, sweep - 2], path[t]) for t in range(T))
    # without a reference the first path is one draw from an ordinary SMC run
    np.random.seed(0)
    out = particle_gibbs.particle_gibbs(observations, model.initial, model.transition, model.emission, model.proposal, K, 2)
    assert all(x.shape == (B, 2, d) for x in out)


# ---- the NumPy sampler against the exact smoother ---------------------------------------------------------------------------
def test_numpy_particle_gibbs_against_the_exact_smoother():
    """The problem of tests/test_gpu_particle_gibbs.py::test_posterior_against_the_exact_smoother (tests/
    particle_gibbs_cases.py: the suite's scalar random walk cut to 25 steps, 256 chains of 8 particles started 60 units
    away from the data, 40 sweeps, 10 discarded), in NumPy float64, chains and sweeps pooled, against the
    Rauch-Tung-Striebel recursion.  Observed over seeds 0 .. 4 of the committed contract:

        with ancestor sampling:     RMSE of the means 0.057 - 0.080, mean relative variance error 0.014 - 0.019,
                                    sweeps that replace x_0 0.629 - 0.636
        without ancestor sampling:  RMSE 1.05 - 1.33, variance error 0.13 - 0.19, sweeps that replace x_0 0.0028 - 0.0038

    The bounds — RMSE < 0.25, variance error < 0.05, replacement > 0.5 with ancestor sampling; replacement < 0.05 and RMSE
    > 0.5 without — keep a factor of two or more from the worst of these, except the replacement rate with ancestor
    sampling (0.63 against 0.5), which does not vary: it is a property of the kernel (K = 8, this model), not of the seed.
    A sampler that forgets to pin the reference, or to re-draw its ancestor, is far outside either set."""
    y = cases.data()
    smooth_m, smooth_p = contract.rts_smoother(y, cases.M0, cases.P0, cases.Q, cases.R)
    start = np.broadcast_to(y + cases.AWAY, (cases.CHAINS, cases.STEPS))
    run = lambda ancestor_sampling: contract.posterior_figures(
        contract.particle_gibbs(y, cases.M0, cases.P0, cases.Q, cases.R, cases.PARTICLES, cases.SWEEPS, start,
                                ancestor_sampling=ancestor_sampling, burn_in=cases.BURN_IN, seed=0), smooth_m, smooth_p)
    rmse, variance, replaced = run(True)
    plain_rmse, plain_variance, plain_replaced = run(False)
    print("\n[numpy particle gibbs] pgas: rmse {:.4f} var rel err {:.4f} replaced {:.4f}; plain: rmse {:.4f} var rel err "
          "{:.4f} replaced {:.4f}".format(rmse, variance, replaced, plain_rmse, plain_variance, plain_replaced))
    assert rmse < cases.RMSE_BOUND and variance < cases.VARIANCE_BOUND and replaced > cases.REPLACED_AT_LEAST
    assert plain_replaced < cases.PLAIN_REPLACED_AT_MOST and plain_rmse > cases.PLAIN_RMSE_AT_LEAST
