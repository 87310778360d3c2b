"""CPU checks of the smoothed continuous state of switching linear-Gaussian models: the NumPy contract of kernel K36
(aesmc_amd/testing/rao_blackwell.py: switching_smooth_combine, switching_state_pass) against the dense Gaussian conditioning
it must agree with, its bound against extended precision, its conventions, the ABI's argument checks, the host logic of
`aesmc_amd.rao_blackwell.conditional_kalman_filter`, `switching_state_smooth` and `switching_smooth_states` on an oracle
provider, the one-regime case where nothing is sampled, and the smoothed mean against the enumeration of all regime
sequences."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as adapted_contract
from aesmc_amd.testing import rao_blackwell as contract
from tests.oracle_provider import OracleKernels

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def _paths(rng, T, B, N, M):
    return [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]


def _against_the_dense_side(model, regimes, ys, out):
    """The largest error over tolerance of a pass against `exact_state_smoother`, trajectory by trajectory."""
    T, (B, N), D = len(ys), regimes[0].shape, model["A"].shape[-1]
    tolerances, worst = out["tolerances"], 0.0
    for b, n in itertools.product(range(B), range(N)):
        sequence = [int(regime[b, n]) for regime in regimes]
        series = [y[b] for y in ys]
        means, covs, crosses = contract.exact_state_smoother(model, sequence, series)
        ell = contract._sequence_log_likelihood(model, sequence, [y[None, :] for y in series])
        pairs = [(out["log_likelihood"][b, n], ell, tolerances["log_likelihood"])]
        for t in range(T):
            pairs.append((out["means"][t][b, n], means[t], tolerances["means"][t]))
            pairs.append((contract.unpack(out["covariances"][t][b, n], D), covs[t], tolerances["covariances"][t]))
            if t < T - 1:
                pairs.append((out["cross_covariances"][t][b, n], crosses[t], tolerances["cross_covariances"][t]))
        for got, want, tolerance in pairs:
            assert np.isfinite(got).all()
            worst = max(worst, float((np.abs(got - want) / (tolerance + 1e-9 * (1.0 + np.abs(want)))).max()))
    return worst


# ---- 1. the mathematics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("M,D,Dy", [(2, 1, 1), (3, 2, 1), (2, 4, 3), (2, 3, 5), (2, 8, 8)])
def test_the_pass_along_given_regimes_is_the_dense_conditioning(M, D, Dy, T):
    """`switching_state_pass` against `exact_state_smoother` (the joint Gaussian of all states and observations conditioned with
    np.linalg): means, covariances, cross-covariances — whose orientation, Cov(z_{t+1,i}, z_{t,l}) at [i,l], this fixes — and
    the conditional filter's log-likelihood against `_sequence_log_likelihood`.  Tolerance: the pass's propagated tolerance
    plus 1e-9 (1 + |value|) for the dense side, the less accurate one.  Measured: the largest error is 3e-15 (at (2,8,8), T = 4), the
    largest share of the allowance 2e-6; no shape needed the dense side checked in extended precision."""
    B, N = 2, 3
    rng = np.random.default_rng([M, D, Dy, T])
    model = contract.example_model(M, D, Dy, seed=1)
    regimes, ys = _paths(rng, T, B, N, M), [rng.standard_normal((B, Dy)) for _ in range(T)]
    out = contract.switching_state_pass(model, regimes, ys)
    assert out["flags"] == 0 and len(out["means"]) == len(out["covariances"]) == T and len(out["cross_covariances"]) == T - 1
    assert np.array_equal(out["means"][-1], out["filtered_means"][-1])      # at T-1 the smoothed moments are the filtered ones
    assert np.array_equal(out["covariances"][-1], out["filtered_covariances"][-1])
    worst = _against_the_dense_side(model, regimes, ys, out)
    print("largest error over allowance", worst)
    assert worst <= 1.0
    if T > 1 and D > 1:      # the orientation is not symmetric: the transpose must fail
        _, _, crosses = contract.exact_state_smoother(model, [int(r[0, 0]) for r in regimes], [y[0] for y in ys])
        assert np.abs(out["cross_covariances"][0][0, 0] - crosses[0].T).max() > 1e-6


@pytest.mark.parametrize("variant,M,D,Dy", [("q", 2, 4, 3), ("s0", 3, 2, 1), ("both", 2, 3, 5)])
def test_singular_noise_and_a_zero_filtered_covariance_stay_finite_and_exact(variant, M, D, Dy):
    """A q column set to 0 (the predicted covariance A P A^T + Q that an RTS step would invert loses rank where P does) and
    s0 = 0 (the filtered P_0 is 0: the P = 0 case): finite, and within the same tolerance of the dense side."""
    B, N, T = 2, 3, 4
    rng = np.random.default_rng([M, D, Dy, 7])
    model = contract.example_model(M, D, Dy, seed=2)
    if variant in ("q", "both"):
        q = model["q"].copy()
        q[:, min(1, D - 1)] = 0.0
        model = dict(model, q=q)
    if variant in ("s0", "both"):
        model = dict(model, s0=np.zeros(D))
    regimes, ys = _paths(rng, T, B, N, M), [rng.standard_normal((B, Dy)) for _ in range(T)]
    out = contract.switching_state_pass(model, regimes, ys)
    assert out["flags"] == 0
    if variant != "q":
        assert (out["filtered_covariances"][0] == 0).all() and (out["covariances"][0] == 0).all()
    worst = _against_the_dense_side(model, regimes, ys, out)
    print("largest error over allowance", worst)
    assert worst <= 1.0


def test_the_exact_mixture_by_hand():
    """`exact_smoothed_state` at T = 1 is Bayes' rule over the regimes on one-step Kalman posteriors; at M = 1 it is
    `exact_state_smoother`."""
    model = contract.example_model(3, 2, 2, seed=3)
    y = np.array([0.3, -1.1])
    mean, cov, lagged = contract.exact_smoothed_state(model, [y])
    ell = np.array([contract._sequence_log_likelihood(model, (s,), [y[None, :]]) for s in range(3)])
    w = model["pi0"] * np.exp(ell)
    w /= w.sum()
    parts = [contract.exact_state_smoother(model, (s,), [y]) for s in range(3)]
    first = sum(w[s] * parts[s][0][0] for s in range(3))
    second = sum(w[s] * (parts[s][1][0] + np.outer(parts[s][0][0], parts[s][0][0])) for s in range(3))
    np.testing.assert_allclose(mean[0], first, rtol=0, atol=1e-14)
    np.testing.assert_allclose(cov[0], second - np.outer(first, first), rtol=0, atol=1e-14)
    assert lagged.shape == (0, 2, 2)
    single = contract.example_model(1, 2, 1, seed=3)
    ys = [np.array([0.2]), np.array([-0.4]), np.array([1.0])]
    mean, cov, lagged = contract.exact_smoothed_state(single, ys)
    m, P, X = contract.exact_state_smoother(single, (0, 0, 0), ys)
    np.testing.assert_allclose(mean, m, rtol=0, atol=1e-14)
    np.testing.assert_allclose(cov, P, rtol=0, atol=1e-14)
    np.testing.assert_allclose(lagged, X + m[1:, :, None] * m[:-1, None, :], rtol=0, atol=1e-14)


# ---- 2. the bound ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 3])      # omega_next None; a rank-deficient Om where Dy < D; a later one
@pytest.mark.parametrize("shape", contract.BACKWARD_SHAPES)
def test_the_bound_holds_against_extended_precision_and_stays_small(shape, steps):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format here: nothing to check against"
    B, _, N, M, D, Dy = shape
    args = contract.example_smooth_combine(B, N, M, D, Dy, steps=steps)
    assert (args[5] is None) == (steps == 1)
    if steps == 2 and Dy < D:
        assert np.linalg.matrix_rank(contract.unpack(args[5], D)[0, 0], tol=1e-9) == Dy
    plain = contract.switching_smooth_combine(*args)
    extended = contract.switching_smooth_combine(*args, dtype=np.longdouble)
    bounds = contract.switching_smooth_combine_bound(*args)
    assert plain[3] == 0
    for name, value, reference, bound, tail in zip(("mean", "cov", "cross"), plain[:3], extended[:3], bounds,
                                                   ((D,), (D * (D + 1) // 2,), (D, D))):
        assert value.shape == (B, N) + tail and bound.shape == value.shape and value.dtype == np.float64, name
        assert np.isfinite(value).all(), name
        assert (np.abs(value - reference.astype(np.float64)) <= bound).all(), name
        assert (bound < 1e-9 * (1.0 + np.abs(value))).all(), name
    # without the cross-covariance: the same smoothed moments, whatever else is handed over
    without = contract.switching_smooth_combine(None, None, args[2], args[3], args[4], None, None)
    assert without[2] is None and without[3] == 0
    assert np.array_equal(without[0], plain[0]) and np.array_equal(without[1], plain[1])
    assert contract.switching_smooth_combine_bound(None, None, args[2], args[3], args[4], None, None)[2] is None


# ---- 3. conventions ----------------------------------------------------------------------------------------------------------------------
def test_conventions_of_the_combination():
    B, N, M, D, Dy = 2, 5, 3, 2, 2
    args = list(contract.example_smooth_combine(B, N, M, D, Dy, steps=2))
    clean = contract.switching_smooth_combine(*args)
    bad = args[1].copy()
    bad[1, 3], bad[0, 0] = M, -1
    got = contract.switching_smooth_combine(args[0], bad, *args[2:])
    gone = np.zeros((B, N), dtype=bool)
    gone[1, 3] = gone[0, 0] = True
    assert got[3] == contract.FLAG_INDEX_OUT_OF_RANGE
    for part, reference in zip(got[:3], clean[:3]):
        assert np.isnan(part[gone]).all() and np.array_equal(part[~gone], reference[~gone])
    bounds = contract.switching_smooth_combine_bound(args[0], bad, *args[2:])
    assert all((bound[gone] == 0).all() for bound in bounds)
    # without the cross-covariance the regimes are not read: no NaN, no flag
    got = contract.switching_smooth_combine(None, None, args[2], args[3], args[4], None, None)
    assert got[3] == 0 and got[2] is None and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # no information (F = 0, lam = 0): the smoothed moments are the filtered ones, bit for bit
    got = contract.switching_smooth_combine(None, None, args[2], np.zeros_like(args[3]), np.zeros_like(args[4]), None, None)
    assert np.array_equal(got[0], args[2][0]) and np.array_equal(got[1], args[2][1])


# ---- 4. the ABI's argument checks -----------------------------------------------------------------------------------------------------------
def _block(_lib, M=2, D=3, Dy=2, **pointers):
    names = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    values = {name: 64 for name in names}
    values.update(pointers)
    return _lib.SwitchingModel(*([values[name] for name in names] + [M, D, Dy]))


def test_the_abi_of_the_combination_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    assert lib.aesmc_version() == 501
    block = lambda **kw: _block(_lib, **kw)
    inputs = {"regime_next": 128, "mean": 136, "cov": 144, "factor": 152, "lam": 160, "omega_next": 168, "cov_next": 176}
    outputs = {"mean_out": 256, "cov_out": 264, "cross_out": 272}

    def combine(model="default", flags=64, B=1, N=4, D=3, **pointers):
        values = dict(inputs, **outputs)
        values.update(pointers)
        model = block() if model == "default" else model
        return lib.aesmc_switching_smooth_combine(None if model is None else ctypes.byref(model), *[
            values[name] for name in ("regime_next", "mean", "cov", "factor", "lam", "omega_next", "cov_next", "mean_out",
                                      "cov_out", "cross_out")], flags, B, N, D, None)

    without = dict(model=None, regime_next=None, omega_next=None, cov_next=None, cross_out=None)
    # every pointer NULL in turn
    for name in ("mean", "cov", "factor", "lam", "mean_out", "cov_out"):
        assert combine(**{name: None}) == 1 and combine(**dict(without, **{name: None})) == 1, name
    assert combine(model=None) == 1 and combine(regime_next=None) == 1 and combine(cov_next=None) == 1
    for name in ("A", "b", "q", "C", "d", "r"):
        assert combine(model=block(**{name: None})) == 1 and combine(model=block(**{name: 68})) == 1, name
    assert combine(model=block(cdf0=None, cdf=None, m0=None, s0=None), B=0) == 0      # (not read)
    assert combine(omega_next=None, B=0) == 0 and combine(flags=None, B=0) == 0         # both are optional
    # without cross_out what only the cross-covariance reads must be NULL too
    assert combine(B=0, **without) == 0
    for name, value in (("model", "default"), ("regime_next", 128), ("omega_next", 168), ("cov_next", 176)):
        assert combine(B=0, **dict(without, **{name: value})) == 1, name
    # sizes
    assert combine(B=-1) == 1 and combine(N=-1) == 1 and combine(D=0) == 1 and combine(D=0, **without) == 1
    assert combine(model=block(M=0)) == 1 and combine(model=block(Dy=0)) == 1
    assert combine(model=block(D=2)) == 1 and combine(D=2) == 1                        # the model's D is the argument's
    # misalignment
    for name, value in list(inputs.items()) + list(outputs.items()):
        assert combine(**{name: value + (2 if name == "regime_next" else 4)}) == 1, name
    assert combine(flags=66) == 1 and combine(mean=140, **without) == 1 and combine(cov_out=268, **without) == 1
    # each output aliasing each input and each other output
    for out in outputs:
        for value in inputs.values():
            assert combine(**{out: value}) == 1, out
        for other, value in outputs.items():
            if other != out:
                assert combine(**{out: value}) == 1, (out, other)
    for out in ("mean_out", "cov_out"):
        for name in ("mean", "cov", "factor", "lam"):
            assert combine(**dict(without, **{out: inputs[name]})) == 1, (out, name)
    assert combine(mean_out=264, **without) == 1
    # the limits
    assert combine(model=block(D=9), D=9) == 2 and combine(model=block(Dy=9)) == 2 and combine(model=block(M=17)) == 2
    assert combine(D=9, **without) == 2
    assert combine(B=1 << 16, N=1 << 16) == 2 and combine(B=1 << 14, N=1 << 12) == 2 and combine(N=1 << 31) == 2
    assert combine(B=1 << 13, N=1 << 13, **without) == 2                               # B N D^2 = 2^32 at D = 8
    # B N = 0 is a no-op, before the limits
    assert combine(B=0) == 0 and combine(N=0) == 0 and combine(B=0, model=block(D=9), D=9) == 0
    assert combine(N=0, **without) == 0 and combine(B=0, D=9, **without) == 0


# ---- 5. the host logic on the oracle provider -----------------------------------------------------------------------------------------------
class StateOracle(OracleKernels):
    """The suite's oracle provider plus K31 - K36 and K21's draw from their NumPy contracts."""

    def __init__(self):
        super().__init__()
        self.calls, self.reads = [], 0

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
        self.calls.append("kalman0" if state is None else "kalman")
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
        scores, flags = contract.switching_backward_scores(log_Pi.numpy(), regime_next.numpy(), factor.numpy(), lam.numpy(),
                                                           tuple(part.numpy() for part in state),
                                                           None if log_w is None else log_w.numpy())
        self._flags |= flags
        return torch.from_numpy(scores)

    def backward_sample(self, log_w, loc, target, scale, u, payload=None):
        assert loc is None and target is None and scale is None and payload is None
        self.calls.append("draw")
        B, K = log_w.shape
        N = u.size(1)
        rows = np.broadcast_to(log_w.numpy()[:, None, :], (B, N, K)).reshape(B * N, K)
        idx, _, flags = contract.categorical_draw(rows, u.numpy().reshape(-1))
        self._flags |= flags
        return torch.from_numpy(idx.reshape(B, N)), None

    def switching_smooth_combine(self, model, regime_next, filtered, factor, lam, omega_next=None, cov_next=None):
        n = lambda t: None if t is None else t.numpy()
        if cov_next is None:
            assert model is None and regime_next is None and omega_next is None
            self.calls.append("combine")
        else:
            self.calls.append("combine+cross0" if omega_next is None else "combine+cross")
        mean, cov, cross, flags = contract.switching_smooth_combine(
            None if model is None else {name: value.numpy() for name, value in model.items()}, n(regime_next),
            (filtered[0].numpy(), filtered[1].numpy()), factor.numpy(), lam.numpy(), n(omega_next), n(cov_next))
        self._flags |= flags
        return torch.from_numpy(mean), torch.from_numpy(cov), None if cross is None else torch.from_numpy(cross)


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = StateOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _torch_model(ops):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS])


def test_the_conditional_filter_and_the_state_smoother_replay_the_contracts_pass(backend):
    from aesmc_amd import rao_blackwell
    T, B, N, M, D, Dy = 5, 3, 7, 3, 2, 2
    TD = D * (D + 1) // 2
    ops = contract.example_model(M, D, Dy, seed=5)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=3)
    regimes = _paths(np.random.default_rng(9), T, B, N, M)
    paths = [torch.from_numpy(regime) for regime in regimes]
    want = contract.switching_state_pass(ops, regimes, [y.numpy() for y in observations])
    assert want["flags"] == 0
    got = rao_blackwell.conditional_kalman_filter(observations, model, paths)
    assert backend.reads == 1 and backend.calls == ["kalman0"] + ["kalman"] * (T - 1)
    assert sorted(got) == ["covariances", "log_likelihood", "means"]
    assert got["log_likelihood"].shape == (B, N) and got["log_likelihood"].dtype == torch.float64
    assert np.array_equal(got["log_likelihood"].numpy(), want["log_likelihood"])
    for t in range(T):
        assert got["means"][t].shape == (B, N, D) and got["covariances"][t].shape == (B, N, TD)
        assert np.array_equal(got["means"][t].numpy(), want["filtered_means"][t])
        assert np.array_equal(got["covariances"][t].numpy(), want["filtered_covariances"][t])
    # the smoother: the launch order, one read, the keys, shapes and dtypes
    backend.calls.clear()
    out = rao_blackwell.switching_state_smooth(observations, model, paths)
    assert backend.reads == 2
    assert backend.calls == ["kalman0"] + ["kalman"] * (T - 1) + ["information0", "combine"] + ["information", "combine"] * (T - 2)
    assert sorted(out) == ["log_likelihood", "smoothed_covariance", "smoothed_mean"]
    backend.calls.clear()
    out = rao_blackwell.switching_state_smooth(observations, model, paths, return_cross_moments=True, return_trajectories=True)
    assert backend.reads == 3
    assert backend.calls == ["kalman0"] + ["kalman"] * (T - 1) + ["information0", "combine+cross0"] + \
        ["information", "combine+cross"] * (T - 2)
    assert sorted(out) == ["covariances", "cross_covariances", "log_likelihood", "means", "smoothed_covariance",
                           "smoothed_cross_moment", "smoothed_mean"]
    assert all(value.dtype == torch.float64 for key in ("means", "covariances", "cross_covariances") for value in out[key])
    assert len(out["means"]) == len(out["covariances"]) == T and len(out["cross_covariances"]) == T - 1
    for t in range(T):
        assert out["means"][t].shape == (B, N, D) and out["covariances"][t].shape == (B, N, TD)
        assert np.array_equal(out["means"][t].numpy(), want["means"][t])
        assert np.array_equal(out["covariances"][t].numpy(), want["covariances"][t])
    for t in range(T - 1):
        assert out["cross_covariances"][t].shape == (B, N, D, D)
        assert np.array_equal(out["cross_covariances"][t].numpy(), want["cross_covariances"][t])
    means = np.stack(want["means"])
    average = means.mean(axis=2)
    second = (contract.unpack(np.stack(want["covariances"]), D) + means[..., :, None] * means[..., None, :]).mean(axis=2)
    lagged = (np.stack(want["cross_covariances"]) + means[1:, ..., :, None] * means[:-1, ..., None, :]).mean(axis=2)
    for key, shape, expected in (("smoothed_mean", (T, B, D), average),
                                 ("smoothed_covariance", (T, B, D, D), second - average[..., :, None] * average[..., None, :]),
                                 ("smoothed_cross_moment", (T - 1, B, D, D), lagged),
                                 ("log_likelihood", (B, N), want["log_likelihood"])):
        assert out[key].shape == shape and out[key].dtype == torch.float64, key
        np.testing.assert_allclose(out[key].numpy(), expected, rtol=0, atol=1e-13, err_msg=key)
    only = rao_blackwell.switching_state_smooth(observations, model, paths, return_cross_moments=True)
    assert sorted(only) == ["log_likelihood", "smoothed_covariance", "smoothed_cross_moment", "smoothed_mean"]
    # float32 observations are widened, as the filter's
    low = rao_blackwell.switching_state_smooth([y.float() for y in observations], model, paths)
    assert low["smoothed_mean"].dtype == torch.float64


def test_one_timestep_and_no_trajectories_launch_nothing_new(backend):
    from aesmc_amd import rao_blackwell
    B, N, M, D, Dy = 2, 4, 3, 2, 2
    model = _torch_model(contract.example_model(M, D, Dy, seed=1))
    observations = model.simulate(1, B, seed=3)
    paths = [torch.from_numpy(_paths(np.random.default_rng(1), 1, B, N, M)[0])]
    out = rao_blackwell.switching_state_smooth(observations, model, paths, return_cross_moments=True, return_trajectories=True)
    assert backend.calls == ["kalman0"]                                                   # T == 1: no K34, no K36
    assert out["smoothed_cross_moment"].shape == (0, B, D, D) and out["cross_covariances"] == []
    assert torch.equal(out["smoothed_mean"][0], out["means"][0].mean(dim=1))
    backend.calls.clear()
    observations = model.simulate(3, B, seed=3)
    empty = [torch.empty((B, 0), dtype=torch.int32)] * 3
    out = rao_blackwell.switching_state_smooth(observations, model, empty, return_cross_moments=True, return_trajectories=True)
    filtered = rao_blackwell.conditional_kalman_filter(observations, model, empty)
    assert backend.calls == []                                                            # N == 0: nothing launched
    assert out["smoothed_mean"].shape == (3, B, D) and not out["smoothed_mean"].any()
    assert out["smoothed_covariance"].shape == (3, B, D, D) and out["smoothed_cross_moment"].shape == (2, B, D, D)
    assert out["log_likelihood"].shape == (B, 0) and filtered["log_likelihood"].shape == (B, 0)
    assert [m.shape for m in out["means"]] == [(B, 0, D)] * 3 and [c.shape for c in out["covariances"]] == [(B, 0, 3)] * 3
    assert [x.shape for x in out["cross_covariances"]] == [(B, 0, D, D)] * 2
    assert [m.shape for m in filtered["means"]] == [(B, 0, D)] * 3


def test_refusals_and_a_regime_out_of_range(backend):
    from aesmc_amd import rao_blackwell
    T, B, N, M, D, Dy = 3, 2, 4, 2, 2, 1
    model = _torch_model(contract.example_model(M, D, Dy, seed=6))
    observations = model.simulate(T, B, seed=1)
    paths = [torch.from_numpy(regime) for regime in _paths(np.random.default_rng(2), T, B, N, M)]
    for run in (rao_blackwell.conditional_kalman_filter, rao_blackwell.switching_state_smooth):
        with pytest.raises(ValueError, match="at least one timestep"):
            run([], model, [])
        with pytest.raises(ValueError, match="one tensor per timestep"):
            run(observations, model, paths[:2])
        with pytest.raises(ValueError, match=r"regimes\[1\]"):
            run(observations, model, [paths[0], paths[1].to(torch.int64), paths[2]])
        with pytest.raises(ValueError, match=r"regimes\[2\]"):
            run(observations, model, paths[:2] + [paths[2][:, :3]])
        with pytest.raises(ValueError, match=r"regimes\[0\] must be \(2, 4\)"):
            run(observations, model, [torch.cat([p, p[:1]]) for p in paths])
        with pytest.raises(ValueError, match="observations must be"):
            run([torch.zeros(B, 3, dtype=torch.float64)] * T, model, paths)
        with pytest.raises(NotImplementedError, match="32-bit element arithmetic.*covered: "):
            run(observations, model, [torch.empty((B, (1 << 24) + 1), dtype=torch.int32)] * T)      # (never touched)
    assert backend.calls == []
    # a regime outside [0, M): the whole run is launched, the marker is read once at the end with the flags, and whatever
    # the launches flagged on the way is discarded
    bad = [p.clone() for p in paths]
    bad[1][1, 2] = M
    for run in (rao_blackwell.conditional_kalman_filter, rao_blackwell.switching_state_smooth):
        backend.calls.clear()
        reads = backend.reads
        with pytest.raises(ValueError, match="regimes holds a value outside"):
            run(observations, model, bad)
        assert backend.reads == reads + 1 and backend.calls[:T] == ["kalman0", "kalman", "kalman"]
        assert backend.read_flags(None) == 0
    assert backend.calls[T:] == ["information0", "combine", "information", "combine"]
    backend.calls.clear()
    with pytest.raises(ValueError, match="regimes holds a value outside"):      # K34 and K36 flag it too: discarded
        rao_blackwell.switching_state_smooth(observations, model, bad, return_cross_moments=True)
    assert backend.read_flags(None) == 0


def test_the_keys_of_both_smoothers(backend):
    from aesmc_amd import rao_blackwell
    T, B, K, N, M, D, Dy = 4, 2, 6, 5, 3, 2, 1
    TD = D * (D + 1) // 2
    model = _torch_model(contract.example_model(M, D, Dy, seed=2))
    observations = model.simulate(T, B, seed=4)
    for lookahead in (False, True):
        torch.manual_seed(5)
        np.random.seed(5)      # (the systematic scheme's uniforms are drawn on the host)
        plain, log_z = rao_blackwell.switching_smooth(observations, model, K, num_trajectories=N, lookahead=lookahead)
        assert sorted(plain) == ["regimes", "smoothed_regime_probabilities"]              # unchanged
        torch.manual_seed(5)
        np.random.seed(5)
        out, again = rao_blackwell.switching_smooth_states(observations, model, K, num_trajectories=N, lookahead=lookahead)
        assert sorted(out) == ["log_likelihood", "regimes", "smoothed_covariance", "smoothed_cross_moment", "smoothed_mean",
                               "smoothed_regime_probabilities"]
        assert torch.equal(again, log_z) and all(torch.equal(a, b) for a, b in zip(out["regimes"], plain["regimes"]))
        assert out["smoothed_mean"].shape == (T, B, D) and out["smoothed_covariance"].shape == (T, B, D, D)
        assert out["smoothed_cross_moment"].shape == (T - 1, B, D, D) and out["log_likelihood"].shape == (B, N)
        assert out["smoothed_regime_probabilities"].shape == (T, B, M) and again.shape == (B,)
        full, _ = rao_blackwell.switching_smooth_states(observations, model, K, num_trajectories=N, lookahead=lookahead,
                                                        return_trajectories=True)
        assert sorted(set(full) - set(out)) == ["covariances", "cross_covariances", "means"]
        assert [m.shape for m in full["means"]] == [(B, N, D)] * T and [c.shape for c in full["covariances"]] == [(B, N, TD)] * T
        assert [x.shape for x in full["cross_covariances"]] == [(B, N, D, D)] * (T - 1)
        # the mixture's covariance is a covariance
        assert (torch.linalg.eigvalsh(out["smoothed_covariance"]) > -1e-12).all()


# ---- 6. one regime: nothing is sampled ---------------------------------------------------------------------------------------------------------
def _one_regime_against_the_exact_smoother(ops, ys, out, log_z, tolerances, K):
    """The largest error over tolerance of `switching_smooth_states` with M = 1 against `exact_state_smoother`: the pass's
    propagated tolerances and nothing else.  The mixture formulas add what they must: the covariance is mean(P^s + m m^T) -
    mean mean^T of N equal trajectories (two products of values within tol_m, twice), the cross moment adds m_{t+1} m_t^T.
    The evidence: `switching_pass`'s (K + 4) u (1 + |lse| + log K) per step beside the summed log-weights' tolerance."""
    T, B = len(ys), ys[0].shape[0]
    worst = 0.0
    for b in range(B):
        means, covs, crosses = contract.exact_state_smoother(ops, (0,) * T, [y[b] for y in ys])
        lagged = crosses + means[1:, :, None] * means[:-1, None, :]
        pairs = []
        for t in range(T):
            pairs.append((out["smoothed_mean"][t, b], means[t], tolerances["means"][t]))
            pairs.append((out["smoothed_covariance"][t, b], covs[t],
                          tolerances["covariances"][t] + 4 * np.abs(means[t]).max() * tolerances["means"][t]))
            if t < T - 1:
                reach = np.abs(means).max() * (tolerances["means"][t] + tolerances["means"][t + 1])
                pairs.append((out["smoothed_cross_moment"][t, b], lagged[t], tolerances["cross_covariances"][t] + 2 * reach))
        exact = contract.exact_log_likelihood(ops, [y[b] for y in ys])
        evidence = tolerances["log_likelihood"] + T * (K + 4) * contract.UNIT * (1.0 + abs(exact) + np.log(K))
        pairs.append((log_z[b], exact, evidence))
        pairs.append((out["log_likelihood"][b], exact, tolerances["log_likelihood"]))      # log p(y | s) is log p(y)
        for got, want, tolerance in pairs:
            worst = max(worst, float((np.abs(got.cpu().numpy() - want) / tolerance).max()))
    return worst


@pytest.mark.parametrize("K,N", [(1, 1), (5, 3)])
def test_one_regime_is_the_exact_smoother_for_any_number_of_particles(backend, K, N):
    """With M = 1 nothing is sampled: `switching_smooth_states` against `exact_state_smoother` within the pass's propagated
    tolerances and nothing else (measured: 0.007 of them at the most)."""
    from aesmc_amd import rao_blackwell
    T, B, D, Dy = 5, 2, 3, 2
    ops = contract.example_model(1, D, Dy, seed=7)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=2)
    ys = [y.numpy() for y in observations]
    out, log_z = rao_blackwell.switching_smooth_states(observations, model, K, num_trajectories=N)
    tolerances = contract.switching_state_pass(ops, [np.zeros((B, 1), dtype=np.int32)] * T, ys)["tolerances"]
    worst = _one_regime_against_the_exact_smoother(ops, ys, out, log_z, tolerances, K)
    print("largest error over the propagated tolerance", worst)
    assert worst <= 1.0


# ---- 7. statistics ---------------------------------------------------------------------------------------------------------------------------------
def statistics_case():
    """(ops, one series T x [Dy], the exact smoothed mean [T,D], spread): tests/test_switching_smoother_contract.py's case —
    M = 2, D = 2, Dy = 1, T = 6, simulated from the model.  spread: the largest distance, over the 64 regime sequences, of a
    sequence's conditional mean from the mixture's — the scale of what a misweighted sequence can move."""
    ops = contract.example_model(2, 2, 1, seed=4)
    series = [y[0].numpy() for y in _torch_model(ops).simulate(6, 1, seed=9)]
    exact, _, _ = contract.exact_smoothed_state(ops, series)
    spread = max(float(np.abs(contract.exact_state_smoother(ops, sequence, series)[0] - exact).max())
                 for sequence in itertools.product(range(2), repeat=6))
    return ops, series, exact, spread


def test_the_smoothed_mean_against_the_enumeration_and_beside_the_filtered_one(backend):
    """One series copied to B = 64 rows, K = N = 256: the row-mean of smoothed_mean lies within 4 across-row standard errors
    plus spread / K (the order of the particle approximation's bias, scaled as the sibling scales 1/K for probabilities) of
    the exact E[z_t | y], and closer to it, in summed absolute error, than the row-mean of the filtered means."""
    from aesmc_amd import rao_blackwell
    ops, series, exact, spread = statistics_case()
    B, K, N = 64, 256, 256
    model = _torch_model(ops)
    observations = [torch.from_numpy(np.broadcast_to(y, (B, 1)).copy()) for y in series]
    torch.manual_seed(17)
    np.random.seed(17)
    filtered = rao_blackwell.switching_filter(observations, model, K, resampling="systematic", return_moments=True)
    drawn = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N)
    out = rao_blackwell.switching_state_smooth(observations, model, drawn["regimes"])
    smoothed = out["smoothed_mean"].numpy()                                                 # [T,B,D]
    mean, standard_error = smoothed.mean(axis=1), smoothed.std(axis=1, ddof=1) / np.sqrt(B)
    error, allowance = np.abs(mean - exact), 4 * standard_error + spread / K
    filtered_error = np.abs(filtered["filtered_mean"].numpy().mean(axis=1) - exact)
    print("spread", spread, "largest error", error.max(), "largest ratio", (error / allowance).max(),
          "summed: smoothed", error.sum(), "filtered", filtered_error.sum())
    assert (error <= allowance).all()
    assert error.sum() < filtered_error.sum()
