"""CPU checks of the Rao-Blackwellised filter for switching linear-Gaussian models: the NumPy contract of kernel K31
(aesmc_amd/testing/rao_blackwell.py) against an independent restatement, the Kalman filter and the exact likelihood by
enumeration; the bound against extended precision; the ABI's argument checks; and the host logic of
`aesmc_amd.rao_blackwell.switching_filter` on a provider that adds the contract's step to the suite's oracle provider."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as adapted_contract
from aesmc_amd.testing import rao_blackwell as contract
from tests.oracle_provider import OracleKernels

LOG_2PI = 1.8378770664093453


def _step_cases():
    for shape in contract.STEP_SHAPES:
        for index in ("none", "sorted", "unsorted"):
            yield shape, index, True
        yield shape, "none", False


def _restated(model, state, idx, uniforms, y):
    """The step from np.linalg, per particle, on full symmetric matrices (Joseph-free textbook form)."""
    B, K = uniforms.shape
    M, D = model["A"].shape[0], model["A"].shape[-1]
    Dy = model["C"].shape[-2]
    regime = np.zeros((B, K), dtype=np.int32)
    mean, cov, log_w = np.zeros((B, K, D)), np.zeros((B, K, D, D)), np.zeros((B, K))
    for b in range(B):
        for k in range(K):
            if state is None:
                row = model["cdf0"]
            else:
                j = k if idx is None else idx[b, k]
                row = model["cdf"][state[0][b, j]]
            s = int(np.searchsorted(row[:M - 1], uniforms[b, k], side="right"))
            A, C = model["A"][s], model["C"][s]
            if state is None:
                m, P = model["m0"], np.diag(model["s0"] ** 2)
            else:
                m = A @ state[1][b, j] + model["b"][s]
                P = A @ contract.unpack(state[2][b, j], D) @ A.T + np.diag(model["q"][s] ** 2)
            S = C @ P @ C.T + np.diag(model["r"][s] ** 2)
            e = y[b].astype(np.float64) - C @ m - model["d"][s]
            gain = P @ C.T @ np.linalg.inv(S)
            regime[b, k], mean[b, k], cov[b, k] = s, m + gain @ e, P - gain @ S @ gain.T
            log_w[b, k] = -0.5 * (e @ np.linalg.solve(S, e) + np.linalg.slogdet(S)[1] + Dy * LOG_2PI)
    return regime, mean, cov, log_w


@pytest.mark.parametrize("shape,index,later", list(_step_cases()))
def test_contract_against_an_independent_restatement(shape, index, later):
    model, state, idx, uniforms, y = contract.example_step(*shape, index=index, later=later)
    regime, mean, cov, log_w, flags = contract.switching_kalman_step(model, state, idx, uniforms, y)
    want = _restated(model, state, idx, uniforms, y)
    assert flags == 0 and regime.dtype == np.int32 and np.array_equal(regime, want[0])
    D = shape[3]
    assert cov.shape == shape[:2] + (D * (D + 1) // 2,)
    # np.linalg's inverse and solve of a D x D system of condition below 1e3: 1e-11 leaves three orders of room
    np.testing.assert_allclose(mean, want[1], rtol=0, atol=1e-11)
    np.testing.assert_allclose(contract.unpack(cov, D), want[2], rtol=0, atol=1e-11)
    np.testing.assert_allclose(log_w, want[3], rtol=0, atol=1e-11)


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,index,later", list(_step_cases()))
def test_the_bound_holds_against_extended_precision_and_stays_small(shape, index, later, observation_dtype):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format here: nothing to check against"
    args = contract.example_step(*shape, index=index, later=later, observation_dtype=observation_dtype)
    plain = contract.switching_kalman_step(*args)
    extended = contract.switching_kalman_step(*args, dtype=np.longdouble)
    bounds = contract.switching_kalman_step_bound(*args)
    assert np.array_equal(plain[0], extended[0])
    for value, reference, bound in zip(plain[1:4], extended[1:4], bounds):
        assert np.isfinite(value).all()
        assert (np.abs(value - reference.astype(np.float64)) <= bound).all()
        assert (bound < 1e-10 * (1.0 + np.abs(value))).all()


def _one_regime(D, Dy, seed):
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.standard_normal((D, D)))[0] * 0.7
    C = np.eye(Dy, D) + 0.3 * rng.standard_normal((Dy, D))
    q, r = rng.uniform(0.3, 0.8, D), rng.uniform(0.3, 0.8, Dy)
    m0, s0 = rng.standard_normal(D), rng.uniform(0.5, 1.5, D)
    model = contract.operands([1.0], [[1.0]], m0, s0, A[None], np.zeros((1, D)), q[None], C[None], np.zeros((1, Dy)), r[None])
    return model, (A, C, q, r, m0, s0)


@pytest.mark.parametrize("K", [1, 7])
def test_one_regime_is_the_kalman_filter(K):
    T, B, D, Dy = 6, 3, 3, 2
    model, (A, C, q, r, m0, s0) = _one_regime(D, Dy, 11)
    rng = np.random.default_rng(12)
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    out = contract.switching_pass(ys, model, K, [rng.uniform(size=(B, K)) for _ in range(T)],
                                  [rng.uniform(size=B) for _ in range(T - 1)])
    means, covs, total = adapted_contract.kalman_filter(A, C, q, r, m0, s0, ys)
    # both are exact filters of the same model: the pass's own tolerance is the whole bound (the difference is 0 at K = 1 and
    # a few units of roundoff at K = 7, where the last log-sum-exp runs over seven equal terms)
    tolerance = out["tolerances"]["log_marginal_likelihood"]
    print("difference", np.abs(out["log_marginal_likelihood"] - total).max(), "tolerance", tolerance)
    assert np.abs(out["log_marginal_likelihood"] - total).max() <= tolerance
    for t in range(T):
        np.testing.assert_allclose(out["means"][t], np.broadcast_to(means[t][:, None, :], (B, K, D)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(contract.unpack(out["covariances"][t], D), np.broadcast_to(covs[t], (B, K, D, D)),
                                   rtol=0, atol=1e-12)
    np.testing.assert_allclose(contract.exact_log_likelihood(model, ys), total, rtol=0, atol=1e-11)


def unbiasedness_case():
    """(model, ys [T x [R,Dy]], exact [R]) of the unbiasedness check: ONE series, repeated as R batch rows."""
    M, D, Dy, T, R = 2, 2, 1, 4, 2000
    model = contract.example_model(M, D, Dy, seed=3)
    rng = np.random.default_rng(31)
    series = [rng.standard_normal(Dy) for _ in range(T)]
    exact = contract.exact_log_likelihood(model, series)
    return model, [np.broadcast_to(y, (R, Dy)).copy() for y in series], exact


def test_the_contract_is_unbiased():
    model, ys, exact = unbiasedness_case()
    T, R, K = len(ys), ys[0].shape[0], 16
    rng = np.random.default_rng(32)
    out = contract.switching_pass(ys, model, K, [rng.uniform(size=(R, K)) for _ in range(T)],
                                  [rng.uniform(size=R) for _ in range(T - 1)])
    ratio = np.exp(out["log_marginal_likelihood"] - exact)
    standard_error = ratio.std(ddof=1) / np.sqrt(R)
    print("mean", ratio.mean(), "standard error", standard_error)
    assert standard_error <= 0.01
    assert abs(ratio.mean() - 1.0) <= 4 * standard_error


def test_moments_of_a_pass_by_hand():
    T, B, K, M, D, Dy = 3, 2, 5, 3, 2, 2
    model = contract.example_model(M, D, Dy, seed=4)
    rng = np.random.default_rng(41)
    out = contract.switching_pass([rng.standard_normal((B, Dy)) for _ in range(T)], model, K,
                                  [rng.uniform(size=(B, K)) for _ in range(T)], [rng.uniform(size=B) for _ in range(T - 1)])
    fm, fc, rp = contract.moments(out["regimes"], out["means"], out["covariances"], out["log_weights"], M)
    assert fm.shape == (T, B, D) and fc.shape == (T, B, D, D) and rp.shape == (T, B, M)
    np.testing.assert_allclose(rp.sum(axis=2), 1.0, atol=1e-14)
    t, b = 2, 1
    w = np.exp(out["log_weights"][t][b])
    w /= w.sum()
    mean = sum(w[k] * out["means"][t][b, k] for k in range(K))
    second = sum(w[k] * (contract.unpack(out["covariances"][t][b, k], D) + np.outer(out["means"][t][b, k], out["means"][t][b, k]))
                 for k in range(K))
    np.testing.assert_allclose(fm[t, b], mean, atol=1e-14)
    np.testing.assert_allclose(fc[t, b], second - np.outer(mean, mean), atol=1e-14)


# ---- the ABI's argument checks --------------------------------------------------------------------------------------------
def test_the_abi_rejects_bad_arguments_before_any_launch():
    """NULL or misaligned pointers, negative sizes, extents below 1, an unknown dtype, a state given in part and an output
    that is its input give status 1; D, Dy or M above the limits or B K beyond 32-bit element arithmetic status 2; an empty
    problem is a no-op — no GPU needed."""
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib, rao_blackwell
    lib = _lib.load()
    assert lib.aesmc_version() == 501
    limits = (lib.aesmc_switching_max_latent_dim(), lib.aesmc_switching_max_observation_dim(), lib.aesmc_switching_max_regimes())
    assert limits == (8, 8, 16)
    assert limits == (rao_blackwell.MAX_LATENT_DIM, rao_blackwell.MAX_OBSERVATION_DIM, rao_blackwell.MAX_REGIMES)
    assert limits == (contract.MAX_LATENT_DIM, contract.MAX_OBSERVATION_DIM, contract.MAX_REGIMES)

    def block(M=2, D=3, Dy=2, **pointers):
        values = {name: 64 for name in ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")}
        values.update(pointers)
        return _lib.SwitchingModel(*([values[name] for name in ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")] +
                                     [M, D, Dy]))

    def step(model="default", regime_in=128, mean_in=128, cov_in=128, idx=128, uniforms=128, y=128, regime_out=256,
             mean_out=256, cov_out=256, log_weight=256, flags=64, B=1, K=4, dtype=1):
        model = block() if model == "default" else model
        return lib.aesmc_switching_kalman_step(dtype, None if model is None else ctypes.byref(model), regime_in, mean_in,
                                               cov_in, idx, uniforms, y, regime_out, mean_out, cov_out, log_weight, flags,
                                               B, K, None)

    assert step(model=None) == 1 and step(uniforms=None) == 1 and step(y=None) == 1
    assert step(regime_out=None) == 1 and step(mean_out=None) == 1 and step(cov_out=None) == 1 and step(log_weight=None) == 1
    for name in ("cdf", "m0", "s0", "A", "b", "q", "C", "d", "r"):
        assert step(model=block(**{name: None})) == 1 and step(model=block(**{name: 68})) == 1, name
    assert step(model=block(cdf0=None), B=0) == 0      # (cdf0 is read by the step-0 form only)
    assert step(model=block(cdf0=None), regime_in=None, mean_in=None, cov_in=None) == 1
    assert step(model=block(cdf=None), regime_in=None, mean_in=None, cov_in=None, B=0) == 0
    assert step(B=-1) == 1 and step(K=-1) == 1 and step(dtype=7) == 1
    assert step(model=block(M=0)) == 1 and step(model=block(D=0)) == 1 and step(model=block(Dy=0)) == 1
    assert step(regime_in=None) == 1 and step(mean_in=None) == 1 and step(cov_in=None) == 1      # a state given in part
    assert step(regime_in=130) == 1 and step(mean_in=132) == 1 and step(cov_in=132) == 1 and step(idx=132) == 1
    assert step(uniforms=132) == 1 and step(y=132) == 1 and step(y=130, dtype=0) == 1 and step(flags=66) == 1
    assert step(regime_out=258) == 1 and step(mean_out=260) == 1 and step(cov_out=260) == 1 and step(log_weight=260) == 1
    assert step(regime_out=128) == 1 and step(mean_out=128) == 1 and step(cov_out=128) == 1      # out aliases in
    assert step(model=block(D=9)) == 2 and step(model=block(Dy=9)) == 2 and step(model=block(M=17)) == 2
    assert step(B=1 << 16, K=1 << 16) == 2 and step(B=1 << 14, K=1 << 12) == 2
    assert step(B=0) == 0 and step(K=0) == 0 and step(B=0, model=block(D=9)) == 0
    assert step(idx=None, flags=None, B=0) == 0                                                    # both are optional
    assert step(regime_in=None, mean_in=None, cov_in=None, idx=None, B=0) == 0                      # the step-0 form
    assert step(y=132, dtype=0, B=0) == 0                                                          # float32 rows: 4-byte aligned


# ---- the host logic of switching_filter on the oracle provider --------------------------------------------------------------
class SwitchingOracle(OracleKernels):
    """The suite's oracle provider plus K31 from its NumPy contract."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def switching_limits(self):
        return 8, 8, 16

    def ancestor_index(self, log_w, u):
        if u.dim() != 2 or u.shape != log_w.shape or log_w.size(1) == 1:
            return super().ancestor_index(log_w, u)
        idx, _, flags, _ = adapted_contract.ancestor_index(log_w.numpy(), u.numpy())      # stratified: one uniform per particle
        self._flags |= flags
        return torch.from_numpy(idx)

    def switching_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        return torch.is_tensor(observation) and observation.dim() == 2 and observation.dtype in (torch.float32, torch.float64) \
            and observation.size(1) == observation_dim and latent_dim <= 8 and observation_dim <= 8 and num_regimes <= 16

    def switching_kalman_step(self, model, state, index, uniforms, observation):
        self.calls.append("step0" if state is None else "step")
        regime, mean, cov, log_w, flags = contract.switching_kalman_step(
            {name: value.numpy() for name, value in model.items()},
            None if state is None else tuple(part.numpy() for part in state),
            None if index is None else index.numpy(), uniforms.numpy(), observation.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(log_w)


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = SwitchingOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _torch_model(ops):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in (
        "pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")])


class _Replay:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


@pytest.mark.parametrize("scheme", ["systematic", "stratified"])
def test_filter_keys_shapes_feeds_and_replay(backend, scheme):
    from aesmc_amd import inference, rao_blackwell
    T, B, K, M, D, Dy = 4, 3, 9, 3, 2, 2
    ops = contract.example_model(M, D, Dy, seed=5)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=3)
    assert len(observations) == T and observations[0].shape == (B, Dy) and observations[0].dtype == torch.float64
    gen = torch.Generator().manual_seed(1)
    regime_u = [torch.rand(B, K, dtype=torch.float64, generator=gen) for _ in range(T)]
    shape = (B, K) if scheme == "stratified" else (B,)
    resample_u = [torch.rand(shape, dtype=torch.float64, generator=gen) for _ in range(T - 1)]
    with inference.uniform_feed(_Replay(resample_u)):
        out = rao_blackwell.switching_filter(observations, model, K, resampling=scheme, regime_uniforms=regime_u,
                                             return_moments=True, return_latents=True)
    assert sorted(out) == ["ancestral_indices", "covariances", "filtered_covariance", "filtered_mean", "latents",
                           "log_marginal_likelihood", "log_weight", "log_weights", "means", "regime_probabilities",
                           "regimes"]
    assert out["log_marginal_likelihood"].shape == (B,) and out["log_marginal_likelihood"].dtype == torch.float64
    assert all(s.shape == (B, K) and s.dtype == torch.int32 for s in out["regimes"]) and len(out["regimes"]) == T
    assert all(m.shape == (B, K, D) for m in out["means"]) and all(c.shape == (B, K, 3) for c in out["covariances"])
    assert len(out["ancestral_indices"]) == T - 1 and all(a.dtype == torch.int64 for a in out["ancestral_indices"])
    assert out["log_weight"] is out["log_weights"][-1]
    assert backend.calls == ["step0"] + ["step"] * (T - 1)
    want = contract.switching_pass([y.numpy() for y in observations], ops, K, [u.numpy() for u in regime_u],
                                   [u.numpy() for u in resample_u])
    assert min(want["margins"]) > 1e-9
    for name in ("regimes", "ancestral_indices"):
        assert all(np.array_equal(got.numpy(), expected) for got, expected in zip(out[name], want[name]))
    for name in ("means", "covariances", "log_weights"):
        for got, expected, tolerance in zip(out[name], want[name], want["tolerances"][name]):
            assert np.abs(got.numpy() - expected).max() <= tolerance
    assert np.abs(out["log_marginal_likelihood"].numpy() - want["log_marginal_likelihood"]).max() <= \
        want["tolerances"]["log_marginal_likelihood"]
    # the moments, formed by hand from the stored systems
    fm, fc, rp = contract.moments(want["regimes"], want["means"], want["covariances"], want["log_weights"], M)
    np.testing.assert_allclose(out["filtered_mean"].numpy(), fm, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["filtered_covariance"].numpy(), fc, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["regime_probabilities"].numpy(), rp, rtol=0, atol=1e-12)
    # the genealogy: the last entry is the last stored system, the first follows the composed ancestors
    assert len(out["latents"]) == T and torch.equal(out["latents"][-1], out["regimes"][-1])
    lineage = np.arange(K)[None, :].repeat(B, axis=0)
    for index in reversed(want["ancestral_indices"]):
        lineage = np.take_along_axis(index, lineage, axis=1)
    assert np.array_equal(out["latents"][0].numpy(), np.take_along_axis(want["regimes"][0], lineage, axis=1))
    # a feed of the other scheme's shape
    other = [torch.rand((B,) if scheme == "stratified" else (B, K), dtype=torch.float64) for _ in range(T - 1)]
    with inference.uniform_feed(_Replay(other)), pytest.raises(ValueError, match="uniforms per step"):
        rao_blackwell.switching_filter(observations, model, K, resampling=scheme, regime_uniforms=regime_u)
    # without the switches the optional entries are absent; fresh regime uniforms come from torch's generator
    torch.manual_seed(7)
    first = rao_blackwell.switching_filter(observations, model, K, resampling="stratified")
    torch.manual_seed(7)
    again = rao_blackwell.switching_filter(observations, model, K, resampling="stratified")
    assert "latents" not in first and "filtered_mean" not in first
    assert torch.equal(first["log_marginal_likelihood"], again["log_marginal_likelihood"])


def test_refusals_and_parameter_validation(backend):
    from aesmc_amd import distributed, rao_blackwell
    ops = contract.example_model(2, 2, 1, seed=6)
    model = _torch_model(ops)
    observations = model.simulate(3, 2, seed=1)
    run = lambda **kw: rao_blackwell.switching_filter(kw.pop("observations", observations), kw.pop("model", model),
                                                      kw.pop("K", 4), **kw)
    with pytest.raises(ValueError, match="at least one timestep"):
        run(observations=[])
    with pytest.raises(ValueError, match="num_particles"):
        run(K=0)
    with pytest.raises(ValueError, match="resampling"):
        run(resampling="multinomial")
    with pytest.raises(ValueError, match="one tensor per timestep"):
        run(regime_uniforms=[torch.zeros(2, 4, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"regime_uniforms\[0\]"):
        run(regime_uniforms=[torch.zeros(2, 4)] * 3)
    with pytest.raises(ValueError, match="observations must be"):
        run(observations=[torch.zeros(2, 3, dtype=torch.float64)] * 3)
    with distributed.shard_scope(4, 0, 2), pytest.raises(NotImplementedError, match="shard_scope"):
        run()
    with distributed.shard_scope(4, 0, 2), pytest.raises(NotImplementedError, match="shard_scope"):
        run(resampling="stratified", regime_uniforms=[torch.zeros(2, 4, dtype=torch.float64)] * 3)
    assert backend.calls == []

    def changed(**kw):
        values = {name: torch.from_numpy(ops[name].copy()) for name in ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")}
        values.update(kw)
        return rao_blackwell.SwitchingLinearGaussian(**values)

    with pytest.raises(ValueError, match="negative"):
        run(model=changed(pi0=torch.tensor([1.5, -0.5])))
    with pytest.raises(ValueError, match="sum to 1"):
        run(model=changed(Pi=torch.tensor([[0.5, 0.5], [0.5, 0.5 + 1e-9]], dtype=torch.float64)))
    with pytest.raises(ValueError, match="Pi"):
        run(model=changed(Pi=torch.ones(3, 3) / 3))
    with pytest.raises(ValueError, match="b must be"):
        run(model=changed(b=torch.zeros(3, 2)))
    with pytest.raises(ValueError, match="s0"):
        run(model=changed(s0=torch.ones(3)))
    with pytest.raises(NotImplementedError, match="D > 8.*covered: "):
        run(model=rao_blackwell.SwitchingLinearGaussian([1.0], [[1.0]], torch.zeros(9), 1.0, torch.eye(9)[None],
                                                        torch.zeros(1, 9), torch.ones(1, 9), torch.ones(1, 1, 9),
                                                        torch.zeros(1, 1), torch.ones(1, 1)),
            observations=[torch.zeros(2, 1, dtype=torch.float64)])
    with pytest.raises(NotImplementedError, match="M > 16.*covered: "):
        run(model=changed(pi0=torch.ones(17) / 17, Pi=torch.ones(17, 17) / 17, A=torch.from_numpy(ops["A"][:1].copy()),
                          b=torch.zeros(1, 2), q=torch.ones(1, 2), C=torch.from_numpy(ops["C"][:1].copy()), d=torch.zeros(1, 1),
                          r=torch.ones(1, 1)))
    assert backend.calls == []
    # shared parameters: a leading extent of 1 is the same model as its expansion
    shared = changed(A=torch.from_numpy(ops["A"][:1].copy()), q=torch.from_numpy(ops["q"][:1].copy()))
    expanded = changed(A=torch.from_numpy(ops["A"][:1].copy()).expand(2, 2, 2), q=torch.from_numpy(ops["q"][:1].copy()).expand(2, 2))
    u = [torch.rand(2, 4, dtype=torch.float64) for _ in range(3)]
    np.random.seed(1)
    one = run(model=shared, regime_uniforms=u)
    np.random.seed(1)
    two = run(model=expanded, regime_uniforms=u)
    assert torch.equal(one["log_marginal_likelihood"], two["log_marginal_likelihood"])


def test_a_singular_innovation_raises_and_an_exception_discards_pending_flags(backend):
    from aesmc_amd import rao_blackwell
    singular = rao_blackwell.SwitchingLinearGaussian([1.0], [[1.0]], torch.zeros(2), 1.0, torch.eye(2)[None], torch.zeros(1, 2),
                                                     torch.ones(1, 2), torch.tensor([[[1.0, 0.0], [1.0, 0.0]]]),
                                                     torch.zeros(1, 2), torch.zeros(1, 2))
    observations = [torch.zeros(2, 2, dtype=torch.float64)] * 3
    with pytest.raises(FloatingPointError):
        rao_blackwell.switching_filter(observations, singular, 4)
    with pytest.raises(FloatingPointError):      # one step: no resampling launch to see the NaN — the end's own check
        rao_blackwell.switching_filter(observations[:1], singular, 4)
    # an exception on the way (a replayed uniform of the wrong shape at the last step) discards what was flagged
    bad = [torch.zeros(2, 4, dtype=torch.float64)] * 2 + [torch.zeros(2, 5, dtype=torch.float64)]
    with pytest.raises(ValueError, match=r"regime_uniforms\[2\]"):
        rao_blackwell.switching_filter(observations, singular, 4, regime_uniforms=bad)
    assert backend.read_flags(None) == 0
    model = _torch_model(contract.example_model(2, 2, 1, seed=6))
    out = rao_blackwell.switching_filter(model.simulate(3, 2, seed=1), model, 4)
    assert torch.isfinite(out["log_marginal_likelihood"]).all()


def test_kalman_log_likelihood_against_the_kalman_filter(backend):
    from aesmc_amd import rao_blackwell
    T, B, D, Dy = 5, 3, 3, 2
    ops, (A, C, q, r, m0, s0) = _one_regime(D, Dy, 21)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=2)
    log_p, means, covs = rao_blackwell.kalman_log_likelihood(observations, model)
    want_means, want_covs, want = adapted_contract.kalman_filter(A, C, q, r, m0, s0, [y.numpy() for y in observations])
    assert log_p.shape == (B,) and means.shape == (T, B, D) and covs.shape == (T, B, D, D)
    np.testing.assert_allclose(log_p.numpy(), want, rtol=0, atol=1e-11)
    np.testing.assert_allclose(means.numpy(), want_means, rtol=0, atol=1e-12)
    np.testing.assert_allclose(covs.numpy(), np.broadcast_to(want_covs[:, None], (T, B, D, D)), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="regimes"):
        rao_blackwell.kalman_log_likelihood(observations, _torch_model(contract.example_model(2, D, Dy)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_product_step_refuses_cpu_tensors():
    from aesmc_amd import rao_blackwell
    model = _torch_model(contract.example_model(2, 2, 1, seed=6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rao_blackwell.switching_filter(model.simulate(2, 2, seed=1), model, 4)
