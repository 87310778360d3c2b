"""CPU checks of Rao-Blackwellised backward simulation for switching linear-Gaussian models: the NumPy contract of kernels K34
and K35 (aesmc_amd/testing/rao_blackwell.py: switching_information_step, switching_backward_scores, switching_backward_pass)
against the forward Kalman likelihood it must agree with, its bounds against extended precision, the ABI's argument checks
of both entries, the host logic of `aesmc_amd.rao_blackwell.switching_backward_simulate` and `switching_smooth` on an oracle
provider, and the smoothed regime probabilities against the enumeration of all regime sequences."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as adapted_contract
from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import smoothing as smoothing_contract
from tests.oracle_provider import OracleKernels

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


# ---- 1. the identity with the forward filter ----------------------------------------------------------------------------------------
IDENTITY_EXTENTS = [(2, 1, 1), (3, 2, 1), (2, 4, 3), (4, 5, 2), (2, 8, 8), (3, 8, 1), (2, 3, 5)]


@pytest.mark.parametrize("length", [1, 2, 4])
@pytest.mark.parametrize("M,D,Dy", IDENTITY_EXTENTS)
def test_the_backward_information_and_the_forward_filter_give_the_same_likelihood(M, D, Dy, length):
    """For a particle (m, P) and a future s'_{1..L}, y_{1..L}: c_0 + (score - log w - log Pi) is log p(y_{1..L} | m, P, s'),
    which the forward filter gives as the sum of `switching_kalman_step`'s log-weights forced along that future (`_forced`).
    Tolerance: the sum of the bounds of every launch on either side — the L information steps' on c, the scores', the L
    Kalman steps' on the log-weight — plus one unit of the sums formed here.  (2,4,3) has a q = 0, (4,5,2) has P = 0."""
    B, K, N = 2, 5, 3
    rng = np.random.default_rng([M, D, Dy, length])
    model = contract.example_model(M, D, Dy, seed=1)
    if (M, D, Dy) == (2, 4, 3):
        q = model["q"].copy()
        q[:, 1] = 0.0
        model = dict(model, q=q)
    factor = rng.standard_normal((B, K, D, D))
    cov = contract.pack(factor @ np.swapaxes(factor, -1, -2) / D + 0.1 * np.eye(D))
    if (M, D, Dy) == (4, 5, 2):
        cov = np.zeros_like(cov)
    particles = (rng.integers(0, M, (B, K)).astype(np.int32), rng.standard_normal((B, K, D)), np.ascontiguousarray(cov))
    future = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(length)]
    ys = [rng.standard_normal((B, Dy)) for _ in range(length)]
    info, bound_c = None, np.zeros((B, N))
    for step in range(length - 1, -1, -1):
        om, lam, c, F, flags, margin = contract.switching_information_step(model, future[step], info, ys[step])
        bound_c += contract.switching_information_step_bound(model, future[step], info, ys[step])[2]
        assert flags == 0 and margin > 1e-13      # (no column lies near the threshold: the rule decides as exact arithmetic would)
        info = (om, lam, c)
    log_Pi = _log(model["Pi"])
    scores, flags = contract.switching_backward_scores(log_Pi, future[0], F, lam, particles, None)
    bound_s = contract.switching_backward_scores_bound(log_Pi, future[0], F, lam, particles, None)
    assert flags == 0 and scores.shape == (B, N, K) and np.isfinite(scores).all()
    prior = log_Pi[particles[0][:, None, :], future[0][:, :, None]]
    backward = c[:, :, None] + (scores - prior)
    for n in range(N):
        state, forward, bound_f = particles, np.zeros((B, K)), np.zeros((B, K))
        for step in range(length):
            shim, forced = contract._forced(model, np.broadcast_to(future[step][:, n:n + 1], (B, K)))
            regime, mean, cov_, log_w, flags = contract.switching_kalman_step(shim, state, None, forced, ys[step])
            bound_f += contract.switching_kalman_step_bound(shim, state, None, forced, ys[step])[2]
            assert flags == 0
            state, forward = (regime, mean, cov_), forward + log_w
        tolerance = bound_c[:, n:n + 1] + bound_s[:, n, :] + bound_f + \
            contract.UNIT * (length + 3) * (np.abs(forward) + np.abs(c[:, n:n + 1]) + np.abs(scores[:, n, :]) + np.abs(prior[:, n, :]))
        error = np.abs(backward[:, n, :] - forward)
        assert (error <= tolerance).all(), (error / tolerance).max()


def test_the_factor_of_a_rank_deficient_information_matrix():
    """At t = T-2 the information matrix is A^T C^T R^-1 C A less the noise's share: rank Dy < D.  The columns past the rank
    are zero, F F^T is the matrix to rounding, and the margin says how far the dropped pivots lay from the threshold."""
    model, regime_next, _, y, _, _ = contract.example_backward_step(2, 4, 6, 3, 5, 2)
    om, lam, c, F, flags, margin = contract.switching_information_step(model, regime_next, None, y)
    full = contract.unpack(om, 5)
    assert (np.linalg.matrix_rank(full, tol=1e-9) == 2).all()
    lower = np.tril(contract.unpack(F, 5))
    assert (lower[:, :, :, 2:] == 0).all() and (lower[:, :, np.arange(2), np.arange(2)] > 0).all()
    assert np.abs(lower @ np.swapaxes(lower, -1, -2) - full).max() <= 1e-14 * np.abs(full).max()
    assert 0.5 * 2.0 ** -40 < margin <= 2.0 ** -40      # the dropped pivots are zero to rounding: the threshold's own width away
    # the first step from the zeros: c is the observation's own constant less the noise's determinant, finite
    assert np.isfinite(c).all() and np.isfinite(lam).all()


# ---- 2. the bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("shape", contract.BACKWARD_SHAPES)
def test_the_bounds_hold_against_extended_precision_and_stay_small(shape, steps, observation_dtype):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format here: nothing to check against"
    model, regime_next, info, y, particles, log_w = contract.example_backward_step(*shape, steps=steps,
                                                                                   observation_dtype=observation_dtype)
    plain = contract.switching_information_step(model, regime_next, info, y)
    extended = contract.switching_information_step(model, regime_next, info, y, dtype=np.longdouble)
    bounds = contract.switching_information_step_bound(model, regime_next, info, y)
    assert plain[4] == 0 and plain[5] > 1e-13 and extended[5] > 1e-13      # both keep and drop the same columns
    for name, value, reference, bound in zip(("Om", "lam", "c", "F"), plain[:4], extended[:4], bounds):
        assert np.isfinite(value).all() and bound.shape == value.shape and value.dtype == np.float64, name
        assert (np.abs(value - reference.astype(np.float64)) <= bound).all(), name
        assert (bound < 1e-9 * (1.0 + np.abs(value).max())).all(), name
    assert np.array_equal(plain[3] == 0, extended[3] == 0)
    log_Pi = _log(model["Pi"])
    for weights in (log_w, None):
        args = (log_Pi, regime_next, plain[3], plain[1], particles, weights)
        value, flags = contract.switching_backward_scores(*args)
        reference, _ = contract.switching_backward_scores(*args, dtype=np.longdouble)
        bound = contract.switching_backward_scores_bound(*args)
        assert flags == 0 and value.shape == (shape[0], shape[2], shape[1]) and np.isfinite(value).all()
        assert (np.abs(value - reference.astype(np.float64)) <= bound).all()
        assert (bound < 1e-9 * (1.0 + np.abs(value))).all()


def test_conventions_of_the_scores_and_the_step():
    B, K, N, M, D, Dy = 2, 9, 4, 3, 2, 2
    model, regime_next, info, y, particles, log_w = contract.example_backward_step(B, K, N, M, D, Dy, steps=2)
    om, lam, c, F, flags, _ = contract.switching_information_step(model, regime_next, info, y)
    log_Pi = _log(model["Pi"])
    clean, flags = contract.switching_backward_scores(log_Pi, regime_next, F, lam, particles, log_w)
    assert flags == 0
    # equal weights: nothing is added
    plain, _ = contract.switching_backward_scores(log_Pi, regime_next, F, lam, particles, None)
    np.testing.assert_allclose(clean - plain, np.broadcast_to(log_w[:, None, :], clean.shape), rtol=0, atol=1e-12)
    # a zero transition probability: -inf and not NaN, whatever the rest is — also where the weight is NaN
    blocked = log_Pi.copy()
    blocked[1, 2] = -np.inf
    poisoned = log_w.copy()
    poisoned[0, 0] = np.nan
    got, flags = contract.switching_backward_scores(blocked, regime_next, F, lam, particles, poisoned)
    excluded = (particles[0][:, None, :] == 1) & (regime_next[:, :, None] == 2)
    assert flags == 0 and excluded.any() and np.isneginf(got[excluded]).all()
    nan = np.zeros_like(excluded)
    nan[0, :, 0] = True
    assert np.isnan(got[nan & ~excluded]).all() and np.array_equal(got[~excluded & ~nan], clean[~excluded & ~nan])
    assert (contract.switching_backward_scores_bound(blocked, regime_next, F, lam, particles, log_w)[excluded] == 0).all()
    # regimes outside [0, M) on either side
    bad_next, bad_regime = regime_next.copy(), particles[0].copy()
    bad_next[1, 3], bad_regime[0, 4] = M, -1
    got, flags = contract.switching_backward_scores(log_Pi, bad_next, F, lam, (bad_regime, particles[1], particles[2]), log_w)
    dead = np.zeros((B, N, K), dtype=bool)
    dead[1, 3, :] = dead[0, :, 4] = True
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE and np.isnan(got[dead]).all() and np.array_equal(got[~dead], clean[~dead])
    out = contract.switching_information_step(model, bad_next, info, y)
    assert out[4] == contract.FLAG_INDEX_OUT_OF_RANGE
    for part, reference in zip(out[:4], (om, lam, c, F)):
        assert np.isnan(part[1, 3]).all() and np.array_equal(np.delete(part[1], 3, 0), np.delete(reference[1], 3, 0))
        assert np.array_equal(part[0], reference[0])


def test_the_categorical_draw_is_k21s():
    rng = np.random.default_rng(8)
    B, K, N = 3, 41, 7
    log_w, u = 3 * rng.standard_normal((B, K)), rng.uniform(size=(B, N))
    log_w[1, :5] = -np.inf
    want, flags, _ = smoothing_contract.backward_sample(log_w, None, None, None, u)
    rows = np.broadcast_to(log_w[:, None, :], (B, N, K)).reshape(B * N, K)
    got, margin, bits = contract.categorical_draw(rows, u.reshape(-1))
    assert flags == bits == 0 and np.array_equal(got.reshape(B, N), want) and (margin > 0).all()
    rows = rows.copy()
    rows[2, 3], rows[5] = np.nan, -np.inf
    got, margin, bits = contract.categorical_draw(rows, u.reshape(-1))
    assert bits == contract.FLAG_NAN_LOG_WEIGHT | contract.FLAG_DEGENERATE_ROW and got[2] == K and got[5] == K
    assert np.array_equal(np.delete(got, [2, 5]), np.delete(want.reshape(-1), [2, 5]))


# ---- the ABI's argument checks -------------------------------------------------------------------------------------------------------
def _block(_lib, M=2, D=3, Dy=2, **pointers):
    names = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    values = {name: 64 for name in names}
    values.update(pointers)
    return _lib.SwitchingModel(*([values[name] for name in names] + [M, D, Dy]))


def test_the_abi_of_the_information_step_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    assert lib.aesmc_version() == 501
    block = lambda **kw: _block(_lib, **kw)

    def step(model="default", regime_next=128, omega_in=136, lambda_in=144, c_in=152, y=160, omega_out=256, lambda_out=264,
             c_out=272, factor_out=280, flags=64, B=1, N=4, dtype=1):
        model = block() if model == "default" else model
        return lib.aesmc_switching_information_step(dtype, None if model is None else ctypes.byref(model), regime_next,
                                                    omega_in, lambda_in, c_in, y, omega_out, lambda_out, c_out, factor_out,
                                                    flags, B, N, None)

    assert step(model=None) == 1 and step(regime_next=None) == 1 and step(y=None) == 1
    assert step(omega_out=None) == 1 and step(lambda_out=None) == 1 and step(c_out=None) == 1 and step(factor_out=None) == 1
    for name in ("A", "b", "q", "C", "d", "r"):
        assert step(model=block(**{name: None})) == 1 and step(model=block(**{name: 68})) == 1, name
    assert step(model=block(cdf0=None, cdf=None, m0=None, s0=None), B=0) == 0      # (not read)
    assert step(B=-1) == 1 and step(N=-1) == 1 and step(dtype=7) == 1
    assert step(model=block(M=0)) == 1 and step(model=block(D=0)) == 1 and step(model=block(Dy=0)) == 1
    assert step(omega_in=None) == 1 and step(lambda_in=None) == 1 and step(c_in=None) == 1      # an input given in part
    assert step(regime_next=130) == 1 and step(omega_in=132) == 1 and step(lambda_in=140) == 1 and step(c_in=148) == 1
    assert step(y=164) == 1 and step(y=162, dtype=0) == 1 and step(flags=66) == 1
    assert step(omega_out=260) == 1 and step(lambda_out=268) == 1 and step(c_out=276) == 1 and step(factor_out=284) == 1
    assert step(omega_out=136) == 1 and step(lambda_out=144) == 1 and step(c_out=152) == 1 and step(factor_out=136) == 1
    assert step(factor_out=256) == 1 and step(c_out=264) == 1 and step(omega_out=160) == 1      # aliasing
    assert step(model=block(D=9)) == 2 and step(model=block(Dy=9)) == 2 and step(model=block(M=17)) == 2
    assert step(B=1 << 16, N=1 << 16) == 2 and step(B=1 << 14, N=1 << 12) == 2
    assert step(B=0) == 0 and step(N=0) == 0 and step(B=0, model=block(D=9)) == 0
    assert step(flags=None, B=0) == 0
    assert step(omega_in=None, lambda_in=None, c_in=None, B=0) == 0                                # the first step's form
    assert step(y=164, dtype=0, B=0) == 0                                                          # float32 rows


def test_the_abi_of_the_scores_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()

    def scores(log_Pi=64, regime_next=128, factor=136, lam=144, regime=152, mean=160, cov=168, log_w=176, out=256, flags=64,
               B=1, K=4, N=3, M=2, D=3):
        return lib.aesmc_switching_backward_scores(log_Pi, regime_next, factor, lam, regime, mean, cov, log_w, out, flags, B, K,
                                                   N, M, D, None)

    for name in ("log_Pi", "regime_next", "factor", "lam", "regime", "mean", "cov", "out"):
        assert scores(**{name: None}) == 1, name
    assert scores(log_w=None, B=0) == 0 and scores(flags=None, B=0) == 0                          # both are optional
    for name, value in (("log_Pi", 68), ("regime_next", 130), ("factor", 140), ("lam", 148), ("regime", 154), ("mean", 164),
                        ("cov", 172), ("log_w", 180), ("out", 260), ("flags", 66)):
        assert scores(**{name: value}) == 1, name
    assert scores(B=-1) == 1 and scores(K=-1) == 1 and scores(N=-1) == 1 and scores(M=0) == 1 and scores(D=0) == 1
    for value in (64, 128, 136, 144, 152, 160, 168, 176):
        assert scores(out=value) == 1                                                             # the scores are an operand
    assert scores(D=9) == 2 and scores(M=17) == 2
    assert scores(B=1 << 11, K=1 << 10, N=1 << 10) == 2                                           # B N K = 2^31
    assert scores(B=1 << 16, K=1 << 16, N=1) == 2 and scores(B=1 << 14, K=1, N=1 << 12) == 2 and scores(K=1 << 31) == 2
    assert scores(B=0) == 0 and scores(K=0) == 0 and scores(N=0) == 0 and scores(B=0, D=9) == 0


# ---- 3. the host logic on the oracle provider ------------------------------------------------------------------------------------------
class SmootherOracle(OracleKernels):
    """The suite's oracle provider plus K31 - K35 and K21's draw from their NumPy contracts."""

    def __init__(self):
        super().__init__()
        self.calls, self.reads, self.weights = [], 0, []

    def read_flags(self, device):
        self.reads += 1
        return super().read_flags(device)

    def switching_limits(self):
        return 8, 8, 16

    def ancestor_index(self, log_w, u):
        if u.dim() != 2 or u.shape != log_w.shape or log_w.size(1) == 1:
            return super().ancestor_index(log_w, u)
        idx, _, flags, _ = adapted_contract.ancestor_index(log_w.numpy(), u.numpy())
        self._flags |= flags
        return torch.from_numpy(idx)

    def switching_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        return torch.is_tensor(observation) and observation.dim() == 2 and observation.dtype in (torch.float32, torch.float64) \
            and observation.size(1) == observation_dim and latent_dim <= 8 and observation_dim <= 8 and num_regimes <= 16

    def switching_backward_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles, num_trajectories):
        return self.switching_covers(observation, num_regimes, latent_dim, observation_dim, num_particles) and \
            observation.size(0) * num_trajectories * num_particles <= 0x7fffffff

    @staticmethod
    def _numpy(model, state):
        return ({name: value.numpy() for name, value in model.items()},
                None if state is None else tuple(part.numpy() for part in state))

    def switching_kalman_step(self, model, state, index, uniforms, observation):
        ops, parts = self._numpy(model, state)
        regime, mean, cov, log_w, flags = contract.switching_kalman_step(
            ops, parts, None if index is None else index.numpy(), uniforms.numpy(), observation.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(log_w)

    def switching_lookahead(self, model, log_prior, state, observation, num_particles=None):
        ops, parts = self._numpy(model, state)
        log_w, cdf, flags = contract.switching_lookahead(ops, log_prior.numpy(), parts, observation.numpy(), num_particles)
        self._flags |= flags
        return torch.from_numpy(log_w), torch.from_numpy(cdf)

    def switching_kalman_draw(self, model, state, index, uniforms, cdf, observation):
        ops, parts = self._numpy(model, state)
        regime, mean, cov, ell, flags = contract.switching_kalman_draw(
            ops, parts, None if index is None else index.numpy(), uniforms.numpy(), cdf.numpy(), observation.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(ell)

    def switching_information_step(self, model, regime_next, info, observation):
        self.calls.append("information0" if info is None else "information")
        ops, parts = self._numpy(model, info)
        om, lam, c, F, flags, _ = contract.switching_information_step(ops, regime_next.numpy(), parts, observation.numpy())
        self._flags |= flags
        return torch.from_numpy(om), torch.from_numpy(lam), torch.from_numpy(c), torch.from_numpy(F)

    def switching_backward_scores(self, log_Pi, regime_next, factor, lam, state, log_w=None):
        self.calls.append("scores")
        self.weights.append(log_w)
        scores, flags = contract.switching_backward_scores(log_Pi.numpy(), regime_next.numpy(), factor.numpy(), lam.numpy(),
                                                           tuple(part.numpy() for part in state),
                                                           None if log_w is None else log_w.numpy())
        self._flags |= flags
        return torch.from_numpy(scores)

    def backward_sample(self, log_w, loc, target, scale, u, payload=None):
        assert loc is None and target is None and scale is None and payload is None
        self.calls.append("draw {}x{}".format(*u.shape))
        self.weights.append(log_w)
        B, K = log_w.shape
        N = u.size(1)
        rows = np.broadcast_to(log_w.numpy()[:, None, :], (B, N, K)).reshape(B * N, K)
        idx, _, flags = contract.categorical_draw(rows, u.numpy().reshape(-1))
        self._flags |= flags
        return torch.from_numpy(idx.reshape(B, N)), None


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = SmootherOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _torch_model(ops):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS])


class _Replay:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


def _filtered(pass_out):
    keys = [key for key in ("regimes", "means", "covariances", "log_weights") if key in pass_out]
    return {key: [torch.from_numpy(np.ascontiguousarray(part)) for part in pass_out[key]] for key in keys}


@pytest.mark.parametrize("adapted", [False, True])
def test_replay_gives_the_contracts_trajectories(backend, adapted):
    from aesmc_amd import inference, rao_blackwell
    T, B, K, N, M, D, Dy = 5, 3, 9, 7, 3, 2, 2
    ops = contract.example_model(M, D, Dy, seed=5)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=3)
    ys = [y.numpy() for y in observations]
    rng = np.random.default_rng(12)
    regime_u, resample_u = [rng.uniform(size=(B, K)) for _ in range(T)], [rng.uniform(size=B) for _ in range(T - 1)]
    uniforms = [rng.uniform(size=(B, N)) for _ in range(T)]
    run = rao_blackwell.adapted_switching_filter if adapted else rao_blackwell.switching_filter
    with inference.uniform_feed(_Replay([torch.from_numpy(u) for u in resample_u])):
        filtered = run(observations, model, K, resampling="systematic", regime_uniforms=[torch.from_numpy(u) for u in regime_u])
    reads = backend.reads
    assert ("log_weights" in filtered) != adapted
    out = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N,
                                                    uniforms=[torch.from_numpy(u) for u in uniforms], return_indices=True)
    assert backend.reads == reads + 1                                                               # flags: read once
    assert backend.calls == ["draw {}x{}".format(B, N)] + ["information0", "scores", "draw {}x1".format(B * N)] + \
        ["information", "scores", "draw {}x1".format(B * N)] * (T - 2)
    if adapted:      # equal weights: zeros at the last step, nothing added to the scores
        assert torch.equal(backend.weights[0], torch.zeros(B, K, dtype=torch.float64))
        assert all(w is None for w in backend.weights[1::2])
    else:
        assert backend.weights[0] is filtered["log_weights"][-1] and backend.weights[1] is filtered["log_weights"][-2]
    forward = (contract.adapted_switching_pass if adapted else contract.switching_pass)(ys, ops, K, regime_u, resample_u)
    want = contract.switching_backward_pass(forward, ops, ys, uniforms)
    assert want["flags"] == 0 and sorted(out) == ["indices", "regimes", "smoothed_regime_probabilities"]
    assert len(out["regimes"]) == len(out["indices"]) == T
    for got, expected in zip(out["regimes"], want["regimes"]):
        assert got.dtype == torch.int32 and got.shape == (B, N) and np.array_equal(got.numpy(), expected)
    for got, expected in zip(out["indices"], want["indices"]):
        assert got.dtype == torch.int64 and got.shape == (B, N) and np.array_equal(got.numpy(), expected)
    probabilities = out["smoothed_regime_probabilities"]
    assert probabilities.shape == (T, B, M) and probabilities.dtype == torch.float64
    np.testing.assert_allclose(probabilities.numpy(), want["smoothed_regime_probabilities"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(probabilities.sum(dim=2).numpy(), 1.0, rtol=0, atol=1e-15)
    # the contract's own pass from the filter's dict is the same thing
    again = contract.switching_backward_pass({k: [p.numpy() for p in v] for k, v in _filtered(forward).items()}, ops, ys, uniforms)
    assert all(np.array_equal(a, b) for a, b in zip(again["indices"], want["indices"]))
    assert "indices" not in rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N,
                                                                      uniforms=[torch.from_numpy(u) for u in uniforms])


def test_fresh_uniforms_are_drawn_for_the_last_timestep_first_and_default_to_one_trajectory_per_particle(backend):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 4, 2, 6, 2, 2, 1
    ops = contract.example_model(M, D, Dy, seed=2)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=4)
    filtered = rao_blackwell.switching_filter(observations, model, K, resampling="systematic")
    torch.manual_seed(21)
    fresh = rao_blackwell.switching_backward_simulate(filtered, model, observations, return_indices=True)
    torch.manual_seed(21)
    blocks = [torch.rand((B, K), dtype=torch.float64) for _ in range(T)]      # the first block drawn serves t = T-1
    replay = rao_blackwell.switching_backward_simulate(filtered, model, observations, uniforms=blocks[::-1], return_indices=True)
    assert all(index.shape == (B, K) for index in fresh["indices"])
    assert all(torch.equal(a, b) for a, b in zip(fresh["indices"], replay["indices"]))
    assert all(torch.equal(a, b) for a, b in zip(fresh["regimes"], replay["regimes"]))


def test_refusals_and_parameter_validation(backend):
    from aesmc_amd import distributed, rao_blackwell
    T, B, K = 3, 2, 4
    ops = contract.example_model(2, 2, 1, seed=6)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=1)
    filtered = rao_blackwell.switching_filter(observations, model, K)
    backend.calls.clear()
    u = [torch.rand(B, 5, dtype=torch.float64) for _ in range(T)]
    run = lambda **kw: rao_blackwell.switching_backward_simulate(kw.pop("filtered", filtered), kw.pop("model", model),
                                                                 kw.pop("observations", observations), **kw)
    with pytest.raises(ValueError, match="at least one timestep"):
        run(observations=[])
    with pytest.raises(ValueError, match="one block per timestep"):
        run(uniforms=u[:2], num_trajectories=5)
    with pytest.raises(ValueError, match="must not be negative"):
        run(num_trajectories=-1)
    with pytest.raises(ValueError, match="observations must be"):
        run(observations=[torch.zeros(B, 3, dtype=torch.float64)] * T)
    with pytest.raises(ValueError, match="must hold 3 'means'"):
        run(filtered={key: value for key, value in filtered.items() if key != "means"})
    with pytest.raises(ValueError, match="must hold 3 'regimes'"):
        run(filtered=dict(filtered, regimes=filtered["regimes"][:2]))
    with pytest.raises(ValueError, match="must hold 3 'log_weights'"):
        run(filtered=dict(filtered, log_weights=filtered["log_weights"][:2]))
    with pytest.raises(ValueError, match=r"filtered\['covariances'\]\[1\]"):
        run(filtered=dict(filtered, covariances=[filtered["covariances"][0], filtered["covariances"][1][:, :, :2],
                                                 filtered["covariances"][2]]))
    with pytest.raises(ValueError, match=r"filtered\['regimes'\]\[0\]"):
        run(filtered=dict(filtered, regimes=[r.to(torch.int64) for r in filtered["regimes"]]))
    with pytest.raises(ValueError, match=r"filtered\['regimes'\]\[0\] must be \(3, 4\)"):      # another batch size than the observations'
        run(observations=[torch.zeros(B + 1, 1, dtype=torch.float64)] * T)
    with pytest.raises(ValueError, match=r"uniforms\[2\]"):
        run(uniforms=u[:2] + [torch.rand(B, 6, dtype=torch.float64)], num_trajectories=5)
    with pytest.raises(ValueError, match=r"uniforms\[2\]"):
        run(uniforms=u[:2] + [torch.rand(B, 5)], num_trajectories=5)
    with distributed.shard_scope(4, 0, 2), pytest.raises(NotImplementedError, match="shard_scope"):
        run()
    with pytest.raises(NotImplementedError, match="32-bit element arithmetic.*covered: "):
        run(num_trajectories=1 << 29)
    with pytest.raises(ValueError, match="sum to 1"):
        values = {name: torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS}
        values["Pi"] = torch.tensor([[0.5, 0.5], [0.5, 0.5 + 1e-9]], dtype=torch.float64)
        run(model=rao_blackwell.SwitchingLinearGaussian(**values))
    assert backend.calls == []
    # inside a shard scope a replay is taken
    with distributed.shard_scope(4, 0, 2):
        assert len(run(uniforms=u, num_trajectories=5)["regimes"]) == T
    # no trajectories: empty tensors, nothing launched
    backend.calls.clear()
    out = run(num_trajectories=0, return_indices=True)
    assert backend.calls == [] and all(r.shape == (B, 0) and r.dtype == torch.int32 for r in out["regimes"])
    assert all(i.shape == (B, 0) and i.dtype == torch.int64 for i in out["indices"])
    assert out["smoothed_regime_probabilities"].shape == (T, B, 2)


def test_an_impossible_transition_raises_and_an_exception_discards_pending_flags(backend):
    """Regime 1 cannot be entered from anywhere but every trajectory is made to end there: every score of step T-2 is -inf,
    K21's draw flags the rows, and the one read at the end raises `backward_simulate`'s RuntimeError."""
    from aesmc_amd import rao_blackwell
    T, B, K = 3, 2, 4
    ops = contract.example_model(2, 2, 1, seed=6)
    ops = dict(ops, Pi=np.array([[1.0, 0.0], [1.0, 0.0]]), pi0=np.array([1.0, 0.0]))
    ops = contract.operands(*[ops[name] for name in MODEL_KEYS])
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=1)
    filtered = rao_blackwell.switching_filter(observations, model, K)
    assert all((r == 0).all() for r in filtered["regimes"])
    filtered = dict(filtered, regimes=filtered["regimes"][:-1] + [torch.ones_like(filtered["regimes"][-1])])
    with pytest.raises(RuntimeError, match="no finite maximum"):
        rao_blackwell.switching_backward_simulate(filtered, model, observations)
    assert backend.read_flags(None) == 0
    bad = [torch.rand(B, K, dtype=torch.float64)] * 2 + [torch.rand(B, K + 1, dtype=torch.float64)]
    with pytest.raises(ValueError, match=r"uniforms\[0\]"):      # raised at the LAST step of the loop: the flags of T-2 are pending
        rao_blackwell.switching_backward_simulate(filtered, model, observations, uniforms=bad[::-1])
    assert backend.read_flags(None) == 0


def test_one_regime_and_one_timestep(backend):
    from aesmc_amd import rao_blackwell
    ops = contract.operands([1.0], [[1.0]], np.zeros(2), 1.0, 0.7 * np.eye(2)[None], np.zeros((1, 2)), np.full((1, 2), 0.5),
                            np.ones((1, 1, 2)), np.zeros((1, 1)), np.ones((1, 1)))
    model = _torch_model(ops)
    observations = model.simulate(4, 3, seed=2)
    for lookahead in (False, True):
        out, log_z = rao_blackwell.switching_smooth(observations, model, 5, num_trajectories=6, lookahead=lookahead)
        assert log_z.shape == (3,) and all((r == 0).all() and r.shape == (3, 6) for r in out["regimes"])
        assert torch.equal(out["smoothed_regime_probabilities"], torch.ones(4, 3, 1, dtype=torch.float64))
    # T = 1: the draw by the stored weights alone
    model = _torch_model(contract.example_model(3, 2, 2, seed=1))
    observations = model.simulate(1, 2, seed=3)
    backend.calls.clear()
    torch.manual_seed(3)
    out, log_z = rao_blackwell.switching_smooth(observations, model, 8)
    assert backend.calls == ["draw 2x8"] and len(out["regimes"]) == 1 and out["smoothed_regime_probabilities"].shape == (1, 2, 3)
    assert sorted(out) == ["regimes", "smoothed_regime_probabilities"]


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------------------
def statistics_case():
    """(ops, one series T x [Dy], exact smoothed marginals [T,M]): M = 2, D = 2, Dy = 1, T = 6, simulated from the model."""
    ops = contract.example_model(2, 2, 1, seed=4)
    series = [y[0].numpy() for y in _torch_model(ops).simulate(6, 1, seed=9)]
    return ops, series, contract.exact_regime_marginals(ops, series)


def test_exact_regime_marginals_by_hand():
    ops, series, exact = statistics_case()
    assert exact.shape == (6, 2) and np.abs(exact.sum(axis=1) - 1.0).max() < 1e-14
    # T = 1: Bayes' rule on the prior with the one-step Kalman likelihoods
    ell = np.array([contract._sequence_log_likelihood(ops, (s,), [series[0][None, :]]) for s in range(2)])
    posterior = ops["pi0"] * np.exp(ell)
    np.testing.assert_allclose(contract.exact_regime_marginals(ops, series[:1])[0], posterior / posterior.sum(), rtol=1e-13)
    # and the sum of the joint is the likelihood `exact_log_likelihood` gives
    joint = [np.log(ops["pi0"][a]) + np.log(ops["Pi"][a, b]) +
             contract._sequence_log_likelihood(ops, (a, b), [y[None, :] for y in series[:2]]) for a in range(2) for b in range(2)]
    assert abs(np.log(np.exp(joint).sum()) - contract.exact_log_likelihood(ops, series[:2])) < 1e-12


def test_smoothed_probabilities_against_the_enumeration_and_beside_the_filtered_ones(backend):
    """One series copied to B = 64 rows, K = 256, N = 256: the mean over the rows of the smoothed regime probabilities lies
    within 4 across-row standard errors plus 1/K (the order of the particle approximation's bias) of the exact smoothed
    marginals, and closer to them, in summed absolute error, than the row-average of the filtered probabilities."""
    from aesmc_amd import rao_blackwell
    ops, series, exact = statistics_case()
    B, K, N, T = 64, 256, 256, len(series)
    model = _torch_model(ops)
    observations = [torch.from_numpy(np.broadcast_to(y, (B, 1)).copy()) for y in series]
    torch.manual_seed(17)
    np.random.seed(17)
    filtered = rao_blackwell.switching_filter(observations, model, K, resampling="systematic", return_moments=True)
    out = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N)
    smoothed = out["smoothed_regime_probabilities"].numpy()
    mean = smoothed.mean(axis=1)
    standard_error = smoothed.std(axis=1, ddof=1) / np.sqrt(B)
    error = np.abs(mean - exact)
    print("largest error", error.max(), "largest allowance", (4 * standard_error + 1.0 / K).max(),
          "largest ratio", (error / (4 * standard_error + 1.0 / K)).max())
    assert (error <= 4 * standard_error + 1.0 / K).all()
    filtered_mean = filtered["regime_probabilities"].numpy().mean(axis=1)
    print("summed absolute error: smoothed", error.sum(), "filtered", np.abs(filtered_mean - exact).sum())
    assert error.sum() < np.abs(filtered_mean - exact).sum()
