"""CPU checks of particle Gibbs on the regimes of a switching linear-Gaussian model: the NumPy contract of kernels K37 and
K38 (aesmc_amd/testing/rao_blackwell.py: switching_conditional_ancestor_index, switching_kalman_conditional_step,
conditional_switching_pass) against the parts it is made of, the ABI's argument checks of both entries, the host logic of
`aesmc_amd.rao_blackwell.conditional_switching_filter` and `switching_particle_gibbs` on an oracle provider, and the
invariance of one sweep under the exact joint law of the regime sequences."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import particle_gibbs as gibbs_contract
from aesmc_amd.testing import rao_blackwell as contract
from tests.test_switching_smoother_contract import MODEL_KEYS, SmootherOracle, _block, _torch_model


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


def resampling_case(B, K, M, D, Dy, steps, seed=0):
    """(model, log_Pi, regime_next [B], F [B,TD], lam [B,D], particles, log_w, u) of one conditional resampling step: the
    stored particles of `example_backward_step`, (F, lam) from `steps` information steps along one trajectory per row."""
    model, regime_next, info, y, particles, log_w = contract.example_backward_step(B, K, 1, M, D, Dy, steps=steps, seed=seed)
    _, lam, _, F, flags, margin = contract.switching_information_step(model, regime_next, info, y)
    assert flags == 0 and margin > 1e-13
    u = np.random.default_rng([seed, B, K, M, D, Dy, steps, 37]).uniform(size=(B, K))
    return model, _log(model["Pi"]), regime_next[:, 0].copy(), F[:, 0].copy(), lam[:, 0].copy(), particles, log_w, u


# ---- 1. the contract against its parts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 2, 2, 2, 1), (3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_the_contract_is_k26s_free_slots_and_k35s_scores_for_one_trajectory(shape, steps):
    B, K, M, D, Dy = shape
    model, log_Pi, regime_next, F, lam, particles, log_w, u = resampling_case(B, K, M, D, Dy, steps)
    idx, flags, margins, bound = contract.switching_conditional_ancestor_index(log_w, u, log_Pi, regime_next, F, lam, particles)
    assert flags == 0 and idx.dtype == np.int64 and idx.shape == (B, K) and margins.shape == (B, K) and bound.shape == (B,)
    # the free slots are K26's contract
    free, bits = gibbs_contract.conditional_ancestor_index(log_w, u)
    assert bits == 0 and np.array_equal(idx[:, :K - 1], free[:, :K - 1])
    # the pinned slot is K21's draw from K35's scores with N = 1, bit for bit
    scores, bits = contract.switching_backward_scores(log_Pi, regime_next[:, None], F[:, None, :], lam[:, None, :], particles, log_w)
    want, margin, more = contract.categorical_draw(scores[:, 0, :], u[:, K - 1])
    assert bits == more == 0 and np.array_equal(idx[:, K - 1], want)
    if K > 1:
        np.testing.assert_array_equal(margins[:, K - 1], margin)
    full = contract.switching_backward_scores_bound(log_Pi, regime_next[:, None], F[:, None, :], lam[:, None, :], particles, log_w)
    np.testing.assert_array_equal(bound, full[:, 0, :].max(axis=1))
    assert (bound < 1e-9).all() and ((margins > 0) | (K == 1)).all()
    # without ancestor sampling the pinned slot keeps its ancestor and nothing of the rest is read
    plain, bits, margins, bound = contract.switching_conditional_ancestor_index(log_w, u, None, None, None, None, None)
    assert bits == 0 and (plain[:, K - 1] == K - 1).all() and np.array_equal(plain[:, :K - 1], idx[:, :K - 1])
    assert np.isinf(margins[:, K - 1]).all() and (bound == 0).all()
    if K == 1:
        assert (idx == 0).all()


def test_a_missing_weight_or_a_wrong_transition_term_changes_the_pinned_scores():
    """What the invariance test below would catch, stated directly: the pinned scores carry log w and log Pi[s, s']."""
    B, K, M, D, Dy = 2, 9, 3, 2, 2
    model, log_Pi, regime_next, F, lam, particles, log_w, u = resampling_case(B, K, M, D, Dy, 2)
    args = (regime_next[:, None], F[:, None, :], lam[:, None, :], particles)
    with_w, _ = contract.switching_backward_scores(log_Pi, *args, log_w)
    without, _ = contract.switching_backward_scores(log_Pi, *args, None)
    np.testing.assert_allclose(with_w[:, 0] - without[:, 0], log_w, rtol=0, atol=1e-12)
    prior = log_Pi[particles[0], regime_next[:, None]]
    flat, _ = contract.switching_backward_scores(np.zeros_like(log_Pi), *args, log_w)
    np.testing.assert_allclose(with_w[:, 0] - flat[:, 0], prior, rtol=0, atol=1e-12)


def test_bad_rows_and_impossible_transitions():
    B, K, M, D, Dy = 4, 9, 3, 2, 2
    model, log_Pi, regime_next, F, lam, particles, log_w, u = resampling_case(B, K, M, D, Dy, 2)
    run = lambda **kw: contract.switching_conditional_ancestor_index(
        kw.get("log_w", log_w), u, kw.get("log_Pi", log_Pi), kw.get("regime_next", regime_next), F, lam,
        kw.get("particles", particles))
    clean, flags, _, _ = run()
    assert flags == 0
    # a NaN weight: the whole row; -inf everywhere: the whole row
    poisoned = log_w.copy()
    poisoned[1, 3] = np.nan
    poisoned[2] = -np.inf
    got, flags, margins, _ = run(log_w=poisoned)
    assert flags == contract.FLAG_NAN_LOG_WEIGHT | contract.FLAG_DEGENERATE_ROW
    assert (got[1] == K).all() and (got[2] == K).all() and np.array_equal(got[[0, 3]], clean[[0, 3]])
    assert np.isinf(margins[[1, 2]]).all()
    # every transition into s' impossible: only the pinned slot fails
    blocked = log_Pi.copy()
    blocked[:, regime_next[0]] = -np.inf
    got, flags, _, _ = run(log_Pi=blocked)
    hit = regime_next == regime_next[0]
    assert flags == contract.FLAG_DEGENERATE_ROW and (got[hit, K - 1] == K).all()
    assert np.array_equal(got[:, :K - 1], clean[:, :K - 1]) and np.array_equal(got[~hit, K - 1], clean[~hit, K - 1])
    # one impossible transition: that particle is never the ancestor, the others' scores are unchanged
    single = log_Pi.copy()
    single[particles[0][0, 0], regime_next[0]] = -np.inf
    scores, _ = contract.switching_backward_scores(single, regime_next[:, None], F[:, None], lam[:, None], particles, log_w)
    excluded = (particles[0] == particles[0][0, 0]) & (regime_next[:, None] == regime_next[0])
    assert np.isneginf(scores[:, 0][excluded]).all() and np.isfinite(scores[:, 0][~excluded]).all()
    got, flags, _, _ = run(log_Pi=single)
    assert flags == 0 and not excluded[np.arange(B), got[:, K - 1]].any()
    # a NaN mean: the pinned slot of its row
    mean = particles[1].copy()
    mean[3, 2, 0] = np.nan
    got, flags, _, _ = run(particles=(particles[0], mean, particles[2]))
    assert flags == contract.FLAG_NAN_LOG_WEIGHT and got[3, K - 1] == K and np.array_equal(got[:3], clean[:3])
    assert np.array_equal(got[3, :K - 1], clean[3, :K - 1])
    # a regime outside [0, M) on either side
    regime = particles[0].copy()
    regime[0, 4] = M
    got, flags, _, _ = run(particles=(regime, particles[1], particles[2]))
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT and got[0, K - 1] == K
    assert np.array_equal(got[1:], clean[1:]) and np.array_equal(got[0, :K - 1], clean[0, :K - 1])
    outside = regime_next.copy()
    outside[2] = -1
    got, flags, _, _ = run(regime_next=outside)
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT and got[2, K - 1] == K
    assert np.array_equal(np.delete(got, 2, 0), np.delete(clean, 2, 0))


@pytest.mark.parametrize("later,index", [(False, "none"), (True, "none"), (True, "unsorted")])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 7, 2, 2, 1), (2, 65, 3, 8, 8)])
def test_the_conditional_step_is_k31_with_the_last_slot_forced(shape, later, index):
    B, K, M, D, Dy = shape
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index=index, later=later)
    pinned = np.random.default_rng([B, K, M, 38]).integers(0, M, B).astype(np.int32)
    got = contract.switching_kalman_conditional_step(model, state, idx, uniforms, pinned, y)
    plain = contract.switching_kalman_step(model, state, idx, uniforms, y)
    shim, forced = contract._forced(model, np.broadcast_to(pinned[:, None], (B, K)))
    pin = contract.switching_kalman_step(shim, state, idx, forced, y)
    assert got[4] == 0 and (got[0][:, K - 1] == pinned).all()
    for part, free, last in zip(got[:4], plain[:4], pin[:4]):
        assert np.array_equal(part[:, :K - 1], free[:, :K - 1]) and np.array_equal(part[:, K - 1], last[:, K - 1])
    bounds = contract.switching_kalman_conditional_step_bound(model, state, idx, uniforms, pinned, y)
    extended = contract.switching_kalman_conditional_step(model, state, idx, uniforms, pinned, y, dtype=np.longdouble)
    for value, reference, bound in zip(got[1:4], extended[1:4], bounds):
        assert (np.abs(value - reference.astype(np.float64)) <= bound).all()
    # a pinned regime outside [0, M): that slot alone
    bad = pinned.copy()
    bad[0] = M
    out = contract.switching_kalman_conditional_step(model, state, idx, uniforms, bad, y)
    assert out[4] == contract.FLAG_INDEX_OUT_OF_RANGE and out[0][0, K - 1] == 0 and np.isnan(out[3][0, K - 1])
    assert np.isnan(out[1][0, K - 1]).all() and np.isnan(out[2][0, K - 1]).all()
    keep = np.ones((B, K), dtype=bool)
    keep[0, K - 1] = False
    for part, reference in zip(out[:4], got[:4]):
        assert np.array_equal(part[keep], reference[keep])


# ---- 2. the ABI's argument checks ----------------------------------------------------------------------------------------------------
def test_the_abi_of_the_conditional_resampling_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    assert lib.aesmc_version() == 501
    assert [lib.aesmc_switching_conditional_max_particles(D) for D in (0, 1, 4, 5, 8, 9)] == [0, 8192, 8192, 4096, 4096, 0]

    def call(log_w=64, u=72, log_Pi=128, regime_next=132, factor=136, lam=144, regime=152, mean=160, cov=168, out=256,
             flags=64, B=1, K=4, M=2, D=3):
        return lib.aesmc_switching_conditional_ancestor_index(log_w, u, log_Pi, regime_next, factor, lam, regime, mean, cov,
                                                              out, flags, B, K, M, D, None)

    for name in ("log_w", "u", "log_Pi", "regime_next", "regime", "mean", "cov", "out"):
        assert call(**{name: None}) == 1, name
    assert call(factor=None) == 1 and call(lam=None) == 1                                           # they come together
    assert call(flags=None, B=0) == 0
    assert call(factor=None, lam=None, log_Pi=None, regime_next=None, regime=None, mean=None, cov=None, B=0) == 0
    for name, value in (("log_w", 68), ("u", 76), ("log_Pi", 132), ("regime_next", 134), ("factor", 140), ("lam", 148),
                        ("regime", 154), ("mean", 164), ("cov", 172), ("out", 260), ("flags", 66)):
        assert call(**{name: value}) == 1, name
    assert call(B=-1) == 1 and call(K=-1) == 1 and call(M=0) == 1 and call(D=0) == 1
    for value in (64, 72, 128, 136, 144, 152, 160, 168):
        assert call(out=value) == 1                                                                 # the output is an operand
    assert call(D=9) == 2 and call(M=17) == 2
    assert call(K=8193) == 2 and call(K=4097, D=5) == 2 and call(K=8193, factor=None, lam=None) == 2
    assert call(B=1 << 31) == 2 and call(B=1 << 20, K=1 << 12) == 2
    assert call(B=0) == 0 and call(K=0) == 0 and call(B=0, D=9) == 0 and call(K=0, M=17) == 0


def test_the_abi_of_the_conditional_step_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    block = lambda **kw: _block(_lib, **kw)

    def step(model="default", regime_in=128, mean_in=136, cov_in=144, idx=152, uniforms=160, pinned=164, y=168, regime_out=256,
             mean_out=264, cov_out=272, log_weight=280, flags=64, B=1, K=4, dtype=1):
        model = block() if model == "default" else model
        return lib.aesmc_switching_kalman_conditional_step(dtype, None if model is None else ctypes.byref(model), regime_in,
                                                           mean_in, cov_in, idx, uniforms, pinned, y, regime_out, mean_out,
                                                           cov_out, log_weight, flags, B, K, None)

    assert step(model=None) == 1 and step(uniforms=None) == 1 and step(y=None) == 1 and step(pinned=None) == 1
    assert step(regime_out=None) == 1 and step(mean_out=None) == 1 and step(cov_out=None) == 1 and step(log_weight=None) == 1
    for name in ("m0", "s0", "A", "b", "q", "C", "d", "r", "cdf"):
        assert step(model=block(**{name: None})) == 1 and step(model=block(**{name: 68})) == 1, name
    assert step(regime_in=None) == 1 and step(mean_in=None) == 1 and step(cov_in=None) == 1        # a state given in part
    assert step(regime_in=None, mean_in=None, cov_in=None, idx=None, B=0) == 0                     # the step-0 form
    assert step(regime_in=None, mean_in=None, cov_in=None, model=block(cdf0=None)) == 1
    assert step(B=-1) == 1 and step(K=-1) == 1 and step(dtype=7) == 1
    assert step(model=block(M=0)) == 1 and step(model=block(D=0)) == 1 and step(model=block(Dy=0)) == 1
    assert step(regime_in=130) == 1 and step(mean_in=140) == 1 and step(cov_in=148) == 1 and step(idx=156) == 1
    assert step(uniforms=164) == 1 and step(pinned=166) == 1 and step(y=172) == 1 and step(flags=66) == 1
    assert step(regime_out=258) == 1 and step(mean_out=268) == 1 and step(cov_out=276) == 1 and step(log_weight=284) == 1
    assert step(regime_out=128) == 1 and step(mean_out=136) == 1 and step(cov_out=144) == 1        # aliasing
    assert step(pinned=256) == 1                                                                   # the pinned regimes are an input
    assert step(model=block(D=9)) == 2 and step(model=block(Dy=9)) == 2 and step(model=block(M=17)) == 2
    assert step(B=1 << 16, K=1 << 16) == 2
    assert step(B=0) == 0 and step(K=0) == 0 and step(B=0, model=block(D=9)) == 0 and step(flags=None, B=0) == 0
    assert step(y=172, dtype=0, B=0) == 0                                                          # float32 rows


# ---- 3. the host logic on the oracle provider ------------------------------------------------------------------------------------------
class GibbsOracle(SmootherOracle):
    """`SmootherOracle` (the suite's `OracleKernels` plus K31 - K35 and K21's draw) plus K37 and K38 from their contracts."""

    def switching_conditional_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        return self.switching_covers(observation, num_regimes, latent_dim, observation_dim, num_particles) and \
            num_particles <= (8192 if latent_dim <= 4 else 4096)

    def switching_conditional_ancestor_index(self, log_w, u, log_Pi, regime_next, factor, lam, state):
        self.calls.append("resample" if factor is not None else "resample plain")
        idx, flags, _, _ = contract.switching_conditional_ancestor_index(
            log_w.numpy(), u.numpy(), log_Pi.numpy(), regime_next.numpy(), None if factor is None else factor.numpy(),
            None if lam is None else lam.numpy(), tuple(part.numpy() for part in state))
        self._flags |= flags
        return torch.from_numpy(idx)

    def switching_kalman_conditional_step(self, model, state, index, uniforms, pinned_regime, observation):
        self.calls.append("step")
        ops, parts = self._numpy(model, state)
        regime, mean, cov, log_w, flags = contract.switching_kalman_conditional_step(
            ops, parts, None if index is None else index.numpy(), uniforms.numpy(), pinned_regime.numpy(), observation.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(log_w)


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = GibbsOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def sweep_case(T, B, K, M, D, Dy, seed):
    ops = contract.example_model(M, D, Dy, seed=seed)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=seed + 1)
    rng = np.random.default_rng([seed, T, B, K, 37])
    reference = [rng.integers(0, M, B).astype(np.int32) for _ in range(T)]
    uniforms = [rng.uniform(size=(B, K)) for _ in range(T - 1)] + [rng.uniform(size=(B, 1))]
    regime_u = [rng.uniform(size=(B, K)) for _ in range(T)]
    return ops, model, observations, reference, uniforms, regime_u


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_replayed_uniforms_give_the_contracts_pass(backend, ancestor_sampling):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 5, 3, 9, 3, 2, 2
    ops, model, observations, reference, uniforms, regime_u = sweep_case(T, B, K, M, D, Dy, 5)
    tensors = lambda blocks: [torch.from_numpy(block) for block in blocks]
    path, particles = rao_blackwell.conditional_switching_filter(
        observations, model, K, tensors(reference), ancestor_sampling=ancestor_sampling, uniforms=tensors(uniforms),
        regime_uniforms=tensors(regime_u), return_particles=True)
    assert backend.reads == 1                                                                       # flags: read once
    backward = ["information0"] + ["information"] * (T - 2) if ancestor_sampling else []
    resample = "resample" if ancestor_sampling else "resample plain"
    assert backend.calls == backward + ["step"] + [resample, "step"] * (T - 1) + ["draw {}x1".format(B)]
    want = contract.conditional_switching_pass([y.numpy() for y in observations], ops, K, reference, uniforms, regime_u,
                                               ancestor_sampling=ancestor_sampling)
    assert want["flags"] == 0 and len(path) == T
    assert sorted(particles) == ["ancestral_indices", "covariances", "indices", "log_weights", "means", "regimes"]
    for t in range(T):
        assert path[t].dtype == torch.int32 and path[t].shape == (B,) and np.array_equal(path[t].numpy(), want["path"][t])
        assert np.array_equal(particles["regimes"][t].numpy(), want["regimes"][t])
        assert np.array_equal(particles["regimes"][t][:, K - 1].numpy(), reference[t])              # the reference sits in slot K-1
        assert np.array_equal(particles["log_weights"][t].numpy(), want["log_weights"][t])
        assert particles["indices"][t].dtype == torch.int64 and np.array_equal(particles["indices"][t].numpy(), want["indices"][t])
    for got, expected in zip(particles["ancestral_indices"], want["ancestral_indices"]):
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), expected)
        assert ancestor_sampling or (got[:, K - 1] == K - 1).all()                                  # plain conditional SMC
    if ancestor_sampling:      # the reference's ancestry is broken somewhere (a property of these seeds)
        assert any((a[:, K - 1] != K - 1).any() for a in want["ancestral_indices"])
    assert not isinstance(rao_blackwell.conditional_switching_filter(
        observations, model, K, tensors(reference), uniforms=tensors(uniforms), regime_uniforms=tensors(regime_u)), tuple)


def test_fresh_uniforms_are_drawn_in_the_documented_order(backend):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 4, 2, 6, 2, 2, 1
    ops, model, observations, reference, _, _ = sweep_case(T, B, K, M, D, Dy, 2)
    reference = [torch.from_numpy(r) for r in reference]
    torch.manual_seed(21)
    fresh, particles = rao_blackwell.conditional_switching_filter(observations, model, K, reference, return_particles=True)
    torch.manual_seed(21)
    draw = lambda columns: torch.rand((B, columns), dtype=torch.float64)
    regime_u, uniforms = [draw(K)], []
    for _ in range(1, T):
        uniforms.append(draw(K))
        regime_u.append(draw(K))
    uniforms.append(draw(1))
    replay, again = rao_blackwell.conditional_switching_filter(observations, model, K, reference, uniforms=uniforms,
                                                               regime_uniforms=regime_u, return_particles=True)
    assert all(torch.equal(a, b) for a, b in zip(fresh, replay))
    assert all(torch.equal(a, b) for a, b in zip(particles["ancestral_indices"], again["ancestral_indices"]))
    assert all(torch.equal(a, b) for a, b in zip(particles["regimes"], again["regimes"]))


def test_one_particle_returns_the_reference_and_one_timestep_draws_by_the_weights(backend):
    from aesmc_amd import rao_blackwell
    T, B, M = 4, 3, 3
    ops, model, observations, reference, _, _ = sweep_case(T, B, 1, M, 2, 2, 3)
    reference = [torch.from_numpy(r) for r in reference]
    for ancestor_sampling in (True, False):
        path = rao_blackwell.conditional_switching_filter(observations, model, 1, reference, ancestor_sampling=ancestor_sampling)
        assert all(torch.equal(a, b) for a, b in zip(path, reference))
    backend.calls.clear()
    path = rao_blackwell.conditional_switching_filter(observations[:1], model, 5, reference[:1])
    assert backend.calls == ["step", "draw {}x1".format(B)] and len(path) == 1 and path[0].shape == (B,)


def test_validation_and_refusals(backend):
    from aesmc_amd import distributed, rao_blackwell
    T, B, K = 3, 2, 4
    ops, model, observations, reference, uniforms, regime_u = sweep_case(T, B, K, 2, 2, 1, 6)
    tensors = lambda blocks: [torch.from_numpy(block) for block in blocks]
    reference, uniforms, regime_u = tensors(reference), tensors(uniforms), tensors(regime_u)
    run = lambda **kw: rao_blackwell.conditional_switching_filter(
        kw.pop("observations", observations), kw.pop("model", model), kw.pop("num_particles", K),
        kw.pop("reference", reference), **kw)
    with pytest.raises(ValueError, match="at least one timestep"):
        run(observations=[], reference=[])
    with pytest.raises(ValueError, match="num_particles must be at least 1"):
        run(num_particles=0)
    with pytest.raises(ValueError, match=r"reference must hold one tensor per timestep \(3\), got 2"):
        run(reference=reference[:2])
    with pytest.raises(ValueError, match="reference must hold one tensor per timestep"):
        run(reference=None)
    with pytest.raises(ValueError, match=r"reference\[1\] must be \(2,\) int32"):
        run(reference=[reference[0], reference[1].to(torch.int64), reference[2]])
    with pytest.raises(ValueError, match=r"reference\[2\] must be \(2,\) int32"):
        run(reference=reference[:2] + [torch.zeros(B, 1, dtype=torch.int32)])
    with pytest.raises(ValueError, match="uniforms must hold one block per timestep"):
        run(uniforms=uniforms[:2])
    with pytest.raises(ValueError, match="regime_uniforms must hold one block per timestep"):
        run(regime_uniforms=regime_u[:2])
    with pytest.raises(ValueError, match=r"uniforms\[2\] must be \(2, 1\) float64"):
        run(uniforms=uniforms[:2] + [torch.rand(B, K, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"uniforms\[0\] must be \(2, 4\) float64"):
        run(uniforms=[torch.rand(B, K)] + uniforms[1:])
    with pytest.raises(ValueError, match=r"regime_uniforms\[1\] must be \(2, 4\) float64"):
        run(regime_uniforms=[regime_u[0], torch.rand(B, K + 1, dtype=torch.float64), regime_u[2]])
    with pytest.raises(ValueError, match="observations must be"):
        run(observations=[torch.zeros(B, 3, dtype=torch.float64)] * T)
    with pytest.raises(NotImplementedError, match="num_particles = 8193.*covered: "):
        run(num_particles=8193)
    with distributed.shard_scope(4, 0, 2), pytest.raises(NotImplementedError, match="shard_scope"):
        run()
    with distributed.shard_scope(4, 0, 2), pytest.raises(NotImplementedError, match="shard_scope"):
        run(uniforms=uniforms)
    with distributed.shard_scope(4, 0, 2):      # a full replay is taken
        assert len(run(uniforms=uniforms, regime_uniforms=regime_u)) == T
    with pytest.raises(ValueError, match="sum to 1"):
        values = {name: torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS}
        values["Pi"] = torch.tensor([[0.5, 0.5], [0.5, 0.5 + 1e-9]], dtype=torch.float64)
        run(model=rao_blackwell.SwitchingLinearGaussian(**values))
    with pytest.raises(ValueError, match="0 <= burn_in < num_sweeps"):
        rao_blackwell.switching_particle_gibbs(observations, model, K, 3, burn_in=3)
    # a latent of more than four values: 4096 particles at the most
    wide = _torch_model(contract.example_model(2, 5, 1, seed=1))
    with pytest.raises(NotImplementedError, match="num_particles = 4097 with a latent of 5 values"):
        rao_blackwell.conditional_switching_filter(wide.simulate(T, B, seed=1), wide, 4097, reference)


def test_an_impossible_reference_raises_and_an_exception_discards_pending_flags(backend):
    """Regime 1 cannot be entered from anywhere, and the reference enters it at t = 1: every pinned score of that step is
    -inf, the row is flagged, and the one read at the end raises; a reference outside [0, M) raises too."""
    from aesmc_amd import rao_blackwell
    T, B, K = 3, 2, 4
    ops = contract.example_model(2, 2, 1, seed=6)
    ops = contract.operands(*[dict(ops, Pi=np.array([[1.0, 0.0], [1.0, 0.0]]), pi0=np.array([1.0, 0.0]))[name]
                              for name in MODEL_KEYS])
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=1)
    reference = [torch.zeros(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match="no finite maximum"):
        rao_blackwell.conditional_switching_filter(observations, model, K, reference)
    assert backend.read_flags(None) == 0
    bad = [torch.rand(B, K, dtype=torch.float64), torch.rand(B, K, dtype=torch.float64), torch.rand(B, 2, dtype=torch.float64)]
    with pytest.raises(ValueError, match=r"uniforms\[2\]"):      # raised after the loop: the flags of step 1 are pending
        rao_blackwell.conditional_switching_filter(observations, model, K, reference, uniforms=bad)
    assert backend.read_flags(None) == 0
    outside = [torch.zeros(B, dtype=torch.int32), torch.full((B,), 2, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)]
    with pytest.raises((RuntimeError, FloatingPointError)):
        rao_blackwell.conditional_switching_filter(observations, model, K, outside)
    assert backend.read_flags(None) == 0


def test_particle_gibbs_runs_the_chain_and_counts_the_kept_sweeps(backend):
    from aesmc_amd import rao_blackwell
    T, B, K, M = 4, 3, 5, 3
    ops, model, observations, reference, _, _ = sweep_case(T, B, K, M, 2, 2, 8)
    torch.manual_seed(5)
    np.random.seed(5)
    out = rao_blackwell.switching_particle_gibbs(observations, model, K, 6, reference=[torch.from_numpy(r) for r in reference],
                                                 burn_in=2)
    assert sorted(out) == ["regimes", "smoothed_regime_probabilities"] and len(out["regimes"]) == T
    assert all(r.shape == (B, 4) and r.dtype == torch.int32 for r in out["regimes"])
    probabilities = out["smoothed_regime_probabilities"]
    assert probabilities.shape == (T, B, M) and probabilities.dtype == torch.float64
    frequencies = np.stack([np.stack([(r.numpy() == i).mean(axis=1) for i in range(M)], axis=1) for r in out["regimes"]])
    np.testing.assert_allclose(probabilities.numpy(), frequencies, rtol=0, atol=1e-15)
    # the chain: sweep s starts from the path sweep s - 1 returned
    torch.manual_seed(5)
    np.random.seed(5)
    path = [torch.from_numpy(r) for r in reference]
    for sweep in range(6):
        path = rao_blackwell.conditional_switching_filter(observations, model, K, path)
        if sweep >= 2:
            assert all(torch.equal(out["regimes"][t][:, sweep - 2], path[t]) for t in range(T))
    # without a reference the first path is one trajectory of the smoother
    backend.calls.clear()
    out = rao_blackwell.switching_particle_gibbs(observations, model, K, 1)
    assert "draw {}x1".format(B) in backend.calls and "scores" in backend.calls and out["regimes"][0].shape == (B, 1)


# ---- 4. invariance -------------------------------------------------------------------------------------------------------------------
CHAINS = 8192


def invariance_case():
    """(ops, series T x [Dy], sequences [16,4], probabilities [16]): M = 2, T = 4, D = Dy = 1, a sticky chain, regimes with
    clearly different dynamics, emission and noise; one fixed series."""
    ops = contract.operands([0.6, 0.4], [[0.9, 0.1], [0.1, 0.9]], [0.0], [1.0], [[[0.9]], [[-0.5]]], [[0.0], [0.8]],
                            [[0.3], [0.9]], [[[1.0]], [[0.4]]], [[0.0], [0.5]], [[0.4], [1.0]])
    series = [np.array([0.3]), np.array([-0.9]), np.array([1.1]), np.array([0.2])]
    sequences, probabilities = contract.exact_regime_posterior(ops, series)
    return ops, series, sequences, probabilities


def assert_within_five_standard_errors(paths, sequences, probabilities, what):
    """paths [T, N]: the frequency of every sequence and of every (t, regime) against its exact probability p, each within
    5 sqrt(p (1 - p) / N) — five binomial standard errors; over 24 cells a correct sampler fails with probability 1e-5."""
    T, N = paths.shape
    M = int(sequences.max()) + 1
    codes = (paths * (M ** np.arange(T - 1, -1, -1))[:, None]).sum(axis=0)
    worst = 0.0
    for position, p in enumerate(probabilities):
        frequency = float((codes == position).mean())
        allowed = 5.0 * np.sqrt(p * (1.0 - p) / N)
        worst = max(worst, abs(frequency - p) / allowed)
        assert abs(frequency - p) <= allowed, (what, "sequence", sequences[position], frequency, p)
    for t in range(T):
        for regime in range(M):
            p = float(probabilities[sequences[:, t] == regime].sum())
            frequency = float((paths[t] == regime).mean())
            allowed = 5.0 * np.sqrt(p * (1.0 - p) / N)
            worst = max(worst, abs(frequency - p) / allowed)
            assert abs(frequency - p) <= allowed, (what, "marginal", t, regime, frequency, p)
    print(what, "largest deviation over its allowance", worst)


def test_the_exact_posterior_sums_to_the_marginals():
    ops, series, sequences, probabilities = invariance_case()
    assert sequences.shape == (16, 4) and abs(probabilities.sum() - 1.0) < 1e-14 and (probabilities > 1e-4).all()
    marginals = contract.exact_regime_marginals(ops, series)
    for t in range(4):
        for regime in range(2):
            assert abs(probabilities[sequences[:, t] == regime].sum() - marginals[t, regime]) < 1e-13
    assert tuple(sequences[5]) == (0, 1, 0, 1)      # position = the sequence read as a number in base M


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_one_sweep_leaves_the_exact_posterior_invariant(ancestor_sampling):
    """8192 independent references from the exact joint law, ONE sweep each with K = 3: the new paths have that law."""
    ops, series, sequences, probabilities = invariance_case()
    T, K = len(series), 3
    rng = np.random.default_rng(370 + int(ancestor_sampling))
    start = sequences[rng.choice(len(sequences), size=CHAINS, p=probabilities)]
    reference = [start[:, t].astype(np.int32) for t in range(T)]
    observations = [np.broadcast_to(y, (CHAINS, 1)).copy() for y in series]
    uniforms = [rng.uniform(size=(CHAINS, K)) for _ in range(T - 1)] + [rng.uniform(size=(CHAINS, 1))]
    regime_u = [rng.uniform(size=(CHAINS, K)) for _ in range(T)]
    out = contract.conditional_switching_pass(observations, ops, K, reference, uniforms, regime_u,
                                              ancestor_sampling=ancestor_sampling)
    assert out["flags"] == 0
    paths = np.stack(out["path"])
    assert (paths != np.stack(reference)).any()
    assert_within_five_standard_errors(paths, sequences, probabilities, "ancestor sampling" if ancestor_sampling else "plain")
