"""CPU checks of backward simulation (FFBS): the NumPy contract of aesmc_backward_sample
(aesmc_amd/testing/smoothing.py) against a brute-force loop over every (trajectory, particle) pair, its conventions, the
ABI's argument checks, and the host logic of `aesmc_amd.smoothing` on a provider that adds `backward_sample` from the
contract to the suite's oracle provider."""
import math

import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract
from tests.oracle_provider import OracleKernels

BELOW_ONE = 1.0 - 2.0 ** -53


def brute_force(log_w, loc, target, scale, u):
    """The contract one pair at a time, in Python floats (IEEE float64), with math.exp."""
    B, K = log_w.shape
    M = u.shape[1]
    D = 0 if loc is None else loc.shape[2]
    idx = np.empty((B, M), dtype=np.int64)
    for b in range(B):
        for m in range(M):
            s = []
            for k in range(K):
                q = 0.0
                for d in range(D):
                    inv = 1.0 / float(scale[d] if len(scale) > 1 else scale[0])
                    q += ((float(target[b, m, d]) - float(loc[b, k, d])) * inv) ** 2
                s.append(float(log_w[b, k]) - 0.5 * q)
            top = max(s)
            w = [math.exp(v - top) if v - top > -745.2 else 0.0 for v in s]
            total = 0.0
            for v in w:
                total += v
            thr, run, count = float(u[b, m]) * total, 0.0, 0
            for v in w:
                run += v
                count += run <= thr
            idx[b, m] = min(count, max(k for k in range(K) if w[k] > 0))
    return idx


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,M,D,vector_scale", [(1, 1, 1, 1, False), (2, 5, 4, 2, True), (2, 33, 7, 3, False),
                                                  (1, 70, 3, 1, True)])
def test_contract_equals_a_loop_over_every_pair(dtype, B, K, M, D, vector_scale):
    rng = np.random.RandomState(B * 1000 + K)
    log_w = (2 * rng.randn(B, K)).astype(dtype)
    loc, target = rng.randn(B, K, D).astype(dtype), rng.randn(B, M, D).astype(dtype)
    scale = (0.5 + rng.rand(D if vector_scale else 1)).astype(dtype)
    u = rng.rand(B, M)
    u[0, 0] = 0.0
    payload = rng.randn(B, K, 3).astype(dtype)
    idx, flags, moved = contract.backward_sample(log_w, loc, target, scale, u, payload)
    assert flags == 0 and idx.dtype == np.int64
    np.testing.assert_array_equal(idx, brute_force(log_w, loc, target, scale, u))
    for b in range(B):
        np.testing.assert_array_equal(moved[b], payload[b][idx[b]])


def test_without_a_transition_term_it_is_searchsorted_on_the_cumulative_weights():
    rng = np.random.RandomState(3)
    log_w = (3 * rng.randn(3, 41)).astype(np.float32)
    u = rng.rand(3, 17)
    idx, flags, moved = contract.backward_sample(log_w, None, None, None, u)
    assert flags == 0 and moved is None
    for b in range(3):
        w = np.exp(log_w[b].astype(np.float64) - np.float64(log_w[b].max()))
        c = np.cumsum(w)
        np.testing.assert_array_equal(idx[b], np.searchsorted(c, u[b] * c[-1], "right"))


def test_rows_and_trajectories_are_independent():
    rng = np.random.RandomState(4)
    B, K, M, D = 3, 29, 11, 2
    log_w, loc, target = rng.randn(B, K), rng.randn(B, K, D), rng.randn(B, M, D)
    scale, u = np.array([0.7, 1.3]), rng.rand(B, M)
    idx, _, _ = contract.backward_sample(log_w, loc, target, scale, u)
    perm = rng.permutation(M)
    permuted, _, _ = contract.backward_sample(log_w, loc, target[:, perm], scale, u[:, perm])
    np.testing.assert_array_equal(permuted, idx[:, perm])
    rows = rng.permutation(B)
    moved, _, _ = contract.backward_sample(log_w[rows], loc[rows], target[rows], scale, u[rows])
    np.testing.assert_array_equal(moved, idx[rows])


def test_zero_selects_the_first_particle_of_positive_weight():
    log_w = np.zeros((2, 9))
    log_w[0, :3] = -np.inf          # no weight at all
    log_w[1, :2] = -2000.0          # weight that underflows to zero
    idx, flags, _ = contract.backward_sample(log_w, None, None, None, np.zeros((2, 4)))
    assert flags == 0
    np.testing.assert_array_equal(idx, [[3] * 4, [2] * 4])
    # ... and with a transition term that removes the first particle of positive log-weight
    loc = np.zeros((2, 9, 1))
    loc[:, :5] = 1e6
    idx, flags, _ = contract.backward_sample(log_w, loc, np.zeros((2, 4, 1)), np.ones(1), np.zeros((2, 4)))
    np.testing.assert_array_equal(idx, [[5] * 4, [5] * 4])


def test_the_clamp_keeps_the_last_position_on_a_particle_of_positive_weight():
    rng = np.random.RandomState(5)
    B, K, M = 4, 50, 6
    log_w = rng.randn(B, K)
    log_w[:, 37:] = -np.inf          # a weightless tail
    log_w[1, 30:] = -5000.0          # ... and one that underflows
    idx, flags, _ = contract.backward_sample(log_w, None, None, None, np.full((B, M), BELOW_ONE))
    assert flags == 0
    assert (idx >= 0).all() and (idx < K).all()
    for b in range(B):
        w = contract.backward_weights(log_w[b], None, np.zeros((M, 0)), None)[0]
        assert (w[np.arange(M), idx[b]] > 0).all()
    assert (idx[0] == 36).all() and (idx[1] == 29).all()


def test_nan_and_degenerate_conventions():
    rng = np.random.RandomState(6)
    B, K, M, D = 4, 12, 5, 2
    log_w, loc, target = rng.randn(B, K), rng.randn(B, K, D), rng.randn(B, M, D)
    scale, u = np.ones(1), rng.rand(B, M)
    clean, flags, _ = contract.backward_sample(log_w, loc, target, scale, u)
    assert flags == 0
    bad_w = log_w.copy()
    bad_w[1, 4] = np.nan
    idx, flags, moved = contract.backward_sample(bad_w, loc, target, scale, u, payload=loc)
    assert flags == contract.FLAG_NAN_LOG_WEIGHT
    assert (idx[1] == K).all() and (np.delete(idx, 1, 0) == np.delete(clean, 1, 0)).all()
    np.testing.assert_array_equal(moved[1], np.broadcast_to(loc[1, K - 1], (M, D)))      # idx == K copies particle K - 1
    bad_target = target.copy()
    bad_target[2, 3, 0] = np.nan         # one trajectory only
    idx, flags, _ = contract.backward_sample(log_w, loc, bad_target, scale, u)
    assert flags == contract.FLAG_NAN_LOG_WEIGHT and idx[2, 3] == K
    mask = np.ones((B, M), dtype=bool)
    mask[2, 3] = False
    assert (idx[mask] == clean[mask]).all()
    dead = log_w.copy()
    dead[0] = -np.inf
    idx, flags, _ = contract.backward_sample(dead, loc, target, scale, u)
    assert flags == contract.FLAG_DEGENERATE_ROW and (idx[0] == K).all() and (idx[1:] == clean[1:]).all()
    hot = log_w.copy()
    hot[3, 0] = np.inf
    idx, flags, _ = contract.backward_sample(hot, loc, target, scale, u)
    assert flags == contract.FLAG_DEGENERATE_ROW and (idx[3] == K).all() and (idx[:3] == clean[:3]).all()
    both = bad_w.copy()
    both[0] = -np.inf
    assert contract.backward_sample(both, loc, target, scale, u)[1] == \
        contract.FLAG_NAN_LOG_WEIGHT | contract.FLAG_DEGENERATE_ROW


def test_the_abi_rejects_bad_arguments_before_any_launch():
    """NULL pointers and negative sizes give status 1, a transition term wider than 256 values status 2, an empty
    problem is a no-op — no GPU needed."""
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    view = _lib.View3(16, 4, 1, 1)
    ref = ctypes.byref(view)

    def call(log_w=16, loc=ref, target=ref, scale=16, scale_stride=0, u=16, idx=16, payload=None, out=None, B=1, K=4, M=2,
             D=1, P=0, dtype=0):
        return lib.aesmc_backward_sample(dtype, log_w, loc, target, scale, scale_stride, u, idx, payload, out, None, B, K, M,
                                         D, P, None)

    assert call(log_w=None) == 1 and call(u=None) == 1 and call(idx=None) == 1
    assert call(loc=None) == 1 and call(target=None) == 1 and call(scale=None) == 1
    assert call(loc=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1
    assert call(B=-1) == 1 and call(K=-1) == 1 and call(M=-1) == 1 and call(D=-1) == 1 and call(P=-1) == 1
    assert call(dtype=7) == 1 and call(scale_stride=2) == 1 and call(u=12) == 1
    assert call(P=3) == 1 and call(P=3, payload=ref) == 1            # a tail without its operands
    assert call(K=0) == 1                                            # trajectories and nothing to draw them from
    assert call(D=257) == 2 and call(K=1 << 31) == 2
    assert call(B=0) == 0 and call(M=0) == 0 and call(B=0, D=257) == 0
    assert call(loc=None, target=None, scale=None, D=0, B=0) == 0    # the D == 0 form takes NULL terms


# ---- the host logic on the oracle provider -----------------------------------------------------------------------------
class SmoothingOracle(OracleKernels):
    """The suite's oracle provider plus `backward_sample` from the NumPy contract."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def backward_sample(self, log_w, loc, target, scale, u, payload=None):
        n = lambda t: None if t is None else t.detach().numpy()
        self.calls.append(None if loc is None else tuple(scale.shape))
        idx, flags, moved = contract.backward_sample(n(log_w), n(loc), n(target), n(scale), n(u), n(payload))
        self._flags |= flags
        return torch.from_numpy(idx), None if moved is None else torch.from_numpy(moved)


@pytest.fixture
def smoothing_backend():
    from aesmc_amd import _kernels
    provider = SmoothingOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _filtered(affine=False, dtype=torch.float64, T=5, B=3, K=24, d=2):
    from aesmc_amd import inference
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(d, dtype=dtype, affine=affine).tune_proposal()
    observations = model.simulate(T, B, seed=1)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                          return_latents=False, return_original_latents=True, return_log_weights=True)
    return model, observations, out["original_latents"], out["log_weights"]


def _uniforms(T, B, M, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(B, M, dtype=torch.float64, generator=gen) for _ in range(T)]


@pytest.mark.parametrize("affine", [False, True])
def test_backward_simulate_equals_the_numpy_backward_pass(smoothing_backend, affine):
    from aesmc_amd import smoothing
    model, observations, latents, log_weights = _filtered(affine=affine)
    T, (B, K, d), M = len(latents), latents[0].shape, 10
    uniforms = _uniforms(T, B, M)
    got, indices = smoothing.backward_simulate(latents, log_weights, model.transition, num_trajectories=M,
                                               observations=observations, uniforms=uniforms, return_indices=True)
    A = model.A.detach().numpy()
    x = [torch.as_tensor(latent).detach().numpy() for latent in latents]
    want, want_idx = contract.backward_pass(x, [w.detach().numpy() for w in log_weights], lambda t: x[t] @ A.T,
                                            np.array([float(model.transition_scale)]), [u.numpy() for u in uniforms])
    assert len(got) == T and len(indices) == T
    for t in range(T):
        assert got[t].shape == (B, M, d) and indices[t].shape == (B, M) and indices[t].dtype == torch.int64
        assert not got[t].requires_grad
        if not affine:      # (the affine location is the C oracle's fma chain: the same indices up to a knife edge)
            np.testing.assert_array_equal(indices[t].numpy(), want_idx[t])
            np.testing.assert_array_equal(got[t].numpy(), want[t])
        np.testing.assert_array_equal(got[t].numpy(), np.stack([x[t][b][indices[t][b].numpy()] for b in range(B)]))
    if affine:
        assert np.mean([np.mean(indices[t].numpy() == want_idx[t]) for t in range(T)]) > 0.99
    # the last step has no transition term, every other one the model's one scale value
    assert smoothing_backend.calls == [None] + [(1,)] * (T - 1)


def test_default_draws_come_from_torch_and_leave_numpy_alone(smoothing_backend):
    from aesmc_amd import smoothing
    model, observations, latents, log_weights = _filtered()
    K = latents[0].shape[1]
    np.random.seed(11)
    before = np.random.get_state()
    torch.manual_seed(3)
    first = smoothing.backward_simulate(latents, log_weights, model.transition)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    assert first[0].shape[1] == K                      # M defaults to the number of particles
    torch.manual_seed(3)
    again = smoothing.backward_simulate(latents, log_weights, model.transition)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    other = smoothing.backward_simulate(latents, log_weights, model.transition)
    assert not all(torch.equal(a, b) for a, b in zip(first, other))
    # one [B, M] float64 block per timestep, the last timestep's first
    torch.manual_seed(3)
    T, B = len(latents), latents[0].shape[0]
    blocks = [torch.rand(B, K, dtype=torch.float64) for _ in range(T)][::-1]
    replayed = smoothing.backward_simulate(latents, log_weights, model.transition, uniforms=blocks)
    assert all(torch.equal(a, b) for a, b in zip(first, replayed))


def test_refusals(smoothing_backend):
    from aesmc_amd import distributed, smoothing, state
    full = state.BatchShapeMode.FULLY_EXPANDED
    model, observations, latents, log_weights = _filtered()
    T, (B, K, d) = len(latents), latents[0].shape
    run = lambda transition, **kw: smoothing.backward_simulate(latents, log_weights, transition, num_trajectories=4, **kw)
    tag = lambda dist, mode=full: state.set_batch_shape_mode(dist, mode)
    loc = lambda previous_latents: previous_latents[-1] @ model.A.t()
    with pytest.raises(NotImplementedError, match="dict latents"):
        smoothing.backward_simulate([{"x": x} for x in latents], log_weights, model.transition)
    with pytest.raises(NotImplementedError, match="Laplace"):
        run(lambda previous_latents=None, **kw: tag(torch.distributions.Laplace(loc(previous_latents), 1.0)))
    with pytest.raises(NotImplementedError, match="Independent"):
        run(lambda previous_latents=None, **kw: tag(torch.distributions.Independent(Normal(loc(previous_latents), 1.0), 1)))
    with pytest.raises(NotImplementedError, match="dict"):
        run(lambda previous_latents=None, **kw: {"x": tag(Normal(loc(previous_latents), 1.0))})
    with pytest.raises(NotImplementedError, match="particle-dependent"):
        run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents), torch.ones(B, K, d, dtype=torch.float64))))
    with pytest.raises(NotImplementedError, match="FULLY_EXPANDED"):
        run(lambda previous_latents=None, **kw: tag(Normal(torch.zeros(d, dtype=torch.float64), 1.0),
                                                    state.BatchShapeMode.NOT_EXPANDED))
    with pytest.raises(NotImplementedError, match="location of shape"):
        run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents)[..., :1], 1.0)))
    wide = [torch.zeros(B, K, 257, dtype=torch.float64) for _ in range(T)]
    with pytest.raises(NotImplementedError, match="D > 256"):
        smoothing.backward_simulate(wide, log_weights, lambda previous_latents=None, **kw: tag(Normal(previous_latents[-1], 1.0)))
    # a per-dimension scale is covered
    per_dim = torch.tensor([0.5, 2.0], dtype=torch.float64)
    out = run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents), per_dim)))
    assert smoothing_backend.calls[-1] == (d,) and out[0].shape == (B, 4, d)
    with distributed.shard_scope(2 * B, 0, 2):
        with pytest.raises(NotImplementedError, match="shard_scope"):
            run(model.transition)
        run(model.transition, uniforms=_uniforms(T, B, 4))      # replayed blocks are fine
    with pytest.raises(ValueError, match="one block per timestep"):
        run(model.transition, uniforms=_uniforms(T - 1, B, 4))
    with pytest.raises(ValueError, match="float64"):
        run(model.transition, uniforms=[u.float() for u in _uniforms(T, B, 4)])
    with pytest.raises(ValueError, match="equally long"):
        smoothing.backward_simulate(latents, log_weights[:-1], model.transition)


def test_bad_rows_are_raised_once_at_the_end(smoothing_backend):
    from aesmc_amd import smoothing
    model, observations, latents, log_weights = _filtered()
    poisoned = [w.clone() for w in log_weights]
    poisoned[1][0, 3] = float("nan")
    with pytest.raises(FloatingPointError):
        smoothing.backward_simulate(latents, poisoned, model.transition, num_trajectories=4)
    dead = [w.clone() for w in log_weights]
    dead[2][1] = -float("inf")
    with pytest.raises(RuntimeError, match="no finite maximum"):
        smoothing.backward_simulate(latents, dead, model.transition, num_trajectories=4)
    assert smoothing_backend.read_flags(None) == 0      # nothing is left behind for the next call
    smoothing.backward_simulate(latents, log_weights, model.transition, num_trajectories=4)


def test_smooth_is_infer_followed_by_backward_simulate(smoothing_backend):
    import aesmc_amd
    from aesmc_amd import inference, smoothing
    from aesmc_amd.testing.models import LgssmNd
    assert aesmc_amd.smoothing is smoothing
    model = LgssmNd(2, dtype=torch.float64).tune_proposal()
    observations = model.simulate(4, 3, seed=1)
    torch.manual_seed(9)
    np.random.seed(9)
    trajectories, log_z = smoothing.smooth(observations, model.initial, model.transition, model.emission, model.proposal,
                                           16, num_trajectories=5)
    torch.manual_seed(9)
    np.random.seed(9)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 16,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want = smoothing.backward_simulate(out["original_latents"], out["log_weights"], model.transition, num_trajectories=5,
                                       observations=observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"])
    assert len(trajectories) == 4 and all(torch.equal(a, b) for a, b in zip(trajectories, want))
    assert trajectories[0].shape == (3, 5, 2)
