"""CPU checks of the look-ahead (fully adapted) Rao-Blackwellised filter for switching linear-Gaussian models: the NumPy
contract of kernels K32 and K33 (aesmc_amd/testing/rao_blackwell.py: switching_lookahead, switching_kalman_draw,
adapted_switching_pass) against an independent restatement, its bound against extended precision, the ABI's argument
checks of both entries, the host logic of `aesmc_amd.rao_blackwell.adapted_switching_filter` on an oracle provider, the
known answers (one step, one regime, shared dynamics), exact zeros in the transition matrix, unbiasedness against the
enumeration, and the variance beside the bootstrap's."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as adapted_contract
from aesmc_amd.testing import rao_blackwell as contract
from tests.oracle_provider import OracleKernels

LOG_2PI = 1.8378770664093453
MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


def _cases():
    for shape in contract.STEP_SHAPES:
        yield shape, True
        yield shape, False


def _lookahead_inputs(shape, later, observation_dtype=np.float64):
    model, state, _, _, y = contract.example_step(*shape, later=later, observation_dtype=observation_dtype)
    return model, _log(model["Pi"] if later else model["pi0"]), state, y, shape[1]


def _restated_scores(model, log_prior, state, y, K):
    """g [B,K,M] and l [B,K,M] from np.linalg on full matrices, per particle and regime."""
    B = y.shape[0]
    M, D = model["A"].shape[0], model["A"].shape[-1]
    Dy = model["C"].shape[-2]
    g, ell = np.zeros((B, K, M)), np.zeros((B, K, M))
    for b in range(B):
        for k in range(K):
            for j in range(M):
                A, C = model["A"][j], model["C"][j]
                if state is None:
                    m, P, lp = model["m0"], np.diag(model["s0"] ** 2), log_prior[j]
                else:
                    m = A @ state[1][b, k] + model["b"][j]
                    P = A @ contract.unpack(state[2][b, k], D) @ A.T + np.diag(model["q"][j] ** 2)
                    lp = log_prior[state[0][b, k], j]
                S = C @ P @ C.T + np.diag(model["r"][j] ** 2)
                e = y[b].astype(np.float64) - C @ m - model["d"][j]
                ell[b, k, j] = -0.5 * (e @ np.linalg.solve(S, e) + np.linalg.slogdet(S)[1] + Dy * LOG_2PI)
                g[b, k, j] = lp + ell[b, k, j]
    return g, ell


def _logsumexp(values, axis):
    top = values.max(axis=axis, keepdims=True)
    return np.squeeze(top, axis=axis) + np.log(np.exp(values - top).sum(axis=axis))


@pytest.mark.parametrize("shape,later", list(_cases()))
def test_lookahead_contract_against_an_independent_restatement(shape, later):
    model, log_prior, state, y, K = _lookahead_inputs(shape, later)
    log_w, cdf, flags = contract.switching_lookahead(model, log_prior, state, y, K)
    B, _, M = shape[:3]
    assert flags == 0 and log_w.shape == (B, K) and cdf.shape == (B, K, M) and log_w.dtype == np.float64
    g, _ = _restated_scores(model, log_prior, state, y, K)
    want = _logsumexp(g, axis=2)
    # np.linalg's solve of a system of condition below 1e3 and a sum of at most 16 terms: 1e-11 leaves three orders of room
    np.testing.assert_allclose(log_w, want, rtol=0, atol=1e-11)
    np.testing.assert_allclose(cdf, np.cumsum(np.exp(g - want[:, :, None]), axis=2), rtol=0, atol=1e-11)
    assert (cdf[:, :, -1] == 1.0).all() and (np.diff(cdf, axis=2) >= 0).all()
    if not later:      # the prior is the same for every particle: so is the look-ahead
        assert (log_w == log_w[:, :1]).all() and (cdf == cdf[:, :1]).all()


def _draw_cases():
    for shape in contract.STEP_SHAPES:
        for index in ("none", "sorted", "unsorted"):
            yield shape, index, True
        yield shape, "none", False


@pytest.mark.parametrize("shape,index,later", list(_draw_cases()))
def test_draw_contract_is_the_step_under_the_regime_its_row_gives(shape, later, index):
    model, state, idx, uniforms, y = contract.example_step(*shape, index=index, later=later)
    B, K, M, D, Dy = shape
    _, cdf, _ = contract.switching_lookahead(model, _log(model["Pi"] if later else model["pi0"]), state, y, K)
    regime, mean, cov, ell, flags = contract.switching_kalman_draw(model, state, idx, uniforms, cdf, y)
    rows = cdf if idx is None else cdf[np.arange(B)[:, None], idx]
    want = np.array([[np.searchsorted(rows[b, k, :M - 1], uniforms[b, k], side="right") for k in range(K)] for b in range(B)])
    assert flags == 0 and regime.dtype == np.int32 and np.array_equal(regime, want)
    # the step itself: K31's contract under a chain every row of which is the point mass at that regime
    for b in range(min(B, 2)):
        for k in (0, K - 1):
            s = int(regime[b, k])
            forced = dict(model, cdf0=(np.arange(M) >= s) * 1.0, cdf=np.broadcast_to((np.arange(M) >= s) * 1.0, (M, M)))
            single = None if state is None else tuple(part[b:b + 1] for part in state)
            got = contract.switching_kalman_step(forced, single, None if idx is None else idx[b:b + 1], uniforms[b:b + 1],
                                                 y[b:b + 1])
            assert got[0][0, k] == s
            assert np.array_equal(got[1][0, k], mean[b, k]) and np.array_equal(got[2][0, k], cov[b, k])
            assert got[3][0, k] == ell[b, k]


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,later", list(_cases()))
def test_the_lookahead_bound_holds_against_extended_precision_and_stays_small(shape, later, observation_dtype):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format here: nothing to check against"
    args = _lookahead_inputs(shape, later, observation_dtype)
    plain = contract.switching_lookahead(*args)
    extended = contract.switching_lookahead(*args, dtype=np.longdouble)
    bounds = contract.switching_lookahead_bound(*args)
    for value, reference, bound in zip(plain[:2], extended[:2], bounds):
        assert np.isfinite(value).all() and bound.shape == value.shape
        assert (np.abs(value - reference.astype(np.float64)) <= bound).all()
        assert (bound < 1e-10 * (1.0 + np.abs(value))).all()


@pytest.mark.parametrize("shape", [(2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_scores_and_the_draws_likelihood_agree(shape):
    """l_s of the draw is the look-ahead's g_s - log Pi[s', s], with g_s recovered from the differences of the CDF row:
    within the two bounds combined."""
    model, state, idx, uniforms, y = contract.example_step(*shape, index="unsorted")
    B, K, M = shape[:3]
    log_Pi = _log(model["Pi"])
    log_w, cdf, _ = contract.switching_lookahead(model, log_Pi, state, y, K)
    bound_w, bound_c = contract.switching_lookahead_bound(model, log_Pi, state, y, K)
    regime, _, _, ell, _ = contract.switching_kalman_draw(model, state, idx, uniforms, cdf, y)
    bound_l = contract.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y)[2]
    rows = np.arange(B)[:, None]
    g, bound_g = contract.score_from_cdf(log_w[rows, idx], cdf[rows, idx], regime, bound_w[rows, idx], bound_c[rows, idx])
    log_prior = log_Pi[state[0][rows, idx], regime]
    error = np.abs(ell - (g - log_prior))
    bound = bound_g + bound_l + contract.UNIT * (np.abs(g) + np.abs(log_prior))
    print("largest error", error.max(), "of bound", (error / bound).max(), "largest bound", bound.max())
    assert bound.max() < 1e-6 and (error <= bound).all()


# ---- the ABI's argument checks ---------------------------------------------------------------------------------------------
def _block(_lib, M=2, D=3, Dy=2, **pointers):
    names = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    values = {name: 64 for name in names}
    values.update(pointers)
    return _lib.SwitchingModel(*([values[name] for name in names] + [M, D, Dy]))


def test_the_abi_of_the_lookahead_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    assert lib.aesmc_version() == 501
    block = lambda **kw: _block(_lib, **kw)

    def look(model="default", log_prior=192, regime_in=128, mean_in=136, cov_in=144, y=128, log_weight=256, cdf=264,
             flags=64, B=1, K=4, dtype=1):
        model = block() if model == "default" else model
        return lib.aesmc_switching_lookahead(dtype, None if model is None else ctypes.byref(model), log_prior, regime_in,
                                             mean_in, cov_in, y, log_weight, cdf, flags, B, K, None)

    assert look(model=None) == 1 and look(log_prior=None) == 1 and look(y=None) == 1
    assert look(log_weight=None) == 1 and look(cdf=None) == 1
    for name in ("m0", "s0", "A", "b", "q", "C", "d", "r"):
        assert look(model=block(**{name: None})) == 1 and look(model=block(**{name: 68})) == 1, name
    assert look(model=block(cdf0=None, cdf=None), B=0) == 0      # (the cumulative rows are not read)
    assert look(B=-1) == 1 and look(K=-1) == 1 and look(dtype=7) == 1
    assert look(model=block(M=0)) == 1 and look(model=block(D=0)) == 1 and look(model=block(Dy=0)) == 1
    assert look(regime_in=None) == 1 and look(mean_in=None) == 1 and look(cov_in=None) == 1      # a state given in part
    assert look(regime_in=130) == 1 and look(mean_in=132) == 1 and look(cov_in=132) == 1 and look(log_prior=196) == 1
    assert look(y=132) == 1 and look(y=130, dtype=0) == 1 and look(flags=66) == 1
    assert look(log_weight=260) == 1 and look(cdf=268) == 1
    assert look(cdf=256) == 1 and look(log_weight=136) == 1 and look(cdf=144) == 1 and look(cdf=136) == 1      # aliasing
    assert look(model=block(D=9)) == 2 and look(model=block(Dy=9)) == 2 and look(model=block(M=17)) == 2
    assert look(B=1 << 16, K=1 << 16) == 2 and look(B=1 << 14, K=1 << 12) == 2
    assert look(B=0) == 0 and look(K=0) == 0 and look(B=0, model=block(D=9)) == 0
    assert look(flags=None, B=0) == 0
    assert look(regime_in=None, mean_in=None, cov_in=None, B=0) == 0                               # the step-0 form
    assert look(y=132, dtype=0, B=0) == 0                                                          # float32 rows


def test_the_abi_of_the_draw_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    block = lambda **kw: _block(_lib, **kw)

    def step(model="default", regime_in=128, mean_in=128, cov_in=128, idx=128, uniforms=128, cdf=192, y=128, regime_out=256,
             mean_out=256, cov_out=256, log_weight=256, flags=64, B=1, K=4, dtype=1):
        model = block() if model == "default" else model
        return lib.aesmc_switching_kalman_draw(dtype, None if model is None else ctypes.byref(model), regime_in, mean_in,
                                               cov_in, idx, uniforms, cdf, y, regime_out, mean_out, cov_out, log_weight,
                                               flags, B, K, None)

    assert step(model=None) == 1 and step(uniforms=None) == 1 and step(y=None) == 1 and step(cdf=None) == 1
    assert step(regime_out=None) == 1 and step(mean_out=None) == 1 and step(cov_out=None) == 1 and step(log_weight=None) == 1
    for name in ("m0", "s0", "A", "b", "q", "C", "d", "r"):
        assert step(model=block(**{name: None})) == 1 and step(model=block(**{name: 68})) == 1, name
    assert step(model=block(cdf0=None, cdf=None), B=0) == 0      # (the model's cumulative rows are not read)
    assert step(B=-1) == 1 and step(K=-1) == 1 and step(dtype=7) == 1
    assert step(model=block(M=0)) == 1 and step(model=block(D=0)) == 1 and step(model=block(Dy=0)) == 1
    assert step(regime_in=None) == 1 and step(mean_in=None) == 1 and step(cov_in=None) == 1      # a state given in part
    assert step(regime_in=130) == 1 and step(mean_in=132) == 1 and step(cov_in=132) == 1 and step(idx=132) == 1
    assert step(uniforms=132) == 1 and step(y=132) == 1 and step(y=130, dtype=0) == 1 and step(flags=66) == 1
    assert step(cdf=196) == 1
    assert step(regime_out=258) == 1 and step(mean_out=260) == 1 and step(cov_out=260) == 1 and step(log_weight=260) == 1
    assert step(regime_out=128) == 1 and step(mean_out=128) == 1 and step(cov_out=128) == 1      # out aliases in
    assert step(cdf=256) == 1                                                                     # the rows are an output
    assert step(model=block(D=9)) == 2 and step(model=block(Dy=9)) == 2 and step(model=block(M=17)) == 2
    assert step(B=1 << 16, K=1 << 16) == 2 and step(B=1 << 14, K=1 << 12) == 2
    assert step(B=0) == 0 and step(K=0) == 0 and step(B=0, model=block(D=9)) == 0
    assert step(idx=None, flags=None, B=0) == 0                                                    # both are optional
    assert step(regime_in=None, mean_in=None, cov_in=None, idx=None, B=0) == 0                      # the step-0 form
    assert step(y=132, dtype=0, B=0) == 0
    # K31's entry still reads the model's own rows
    assert lib.aesmc_switching_kalman_step(1, ctypes.byref(block(cdf=None)), 128, 128, 128, 128, 128, 128, 256, 256, 256, 256,
                                           64, 1, 4, None) == 1


# ---- the host logic of adapted_switching_filter on the oracle provider ---------------------------------------------------------
class LookaheadOracle(OracleKernels):
    """The suite's oracle provider plus K32 and K33 from their NumPy contract."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def switching_limits(self):
        return 8, 8, 16

    def ancestor_index(self, log_w, u):
        self.calls.append("resample")
        if u.dim() != 2 or u.shape != log_w.shape or log_w.size(1) == 1:
            return super().ancestor_index(log_w, u)
        idx, _, flags, _ = adapted_contract.ancestor_index(log_w.numpy(), u.numpy())      # stratified: one uniform per particle
        self._flags |= flags
        return torch.from_numpy(idx)

    def switching_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        return torch.is_tensor(observation) and observation.dim() == 2 and observation.dtype in (torch.float32, torch.float64) \
            and observation.size(1) == observation_dim and latent_dim <= 8 and observation_dim <= 8 and num_regimes <= 16

    @staticmethod
    def _numpy(model, state):
        return ({name: value.numpy() for name, value in model.items()},
                None if state is None else tuple(part.numpy() for part in state))

    def switching_lookahead(self, model, log_prior, state, observation, num_particles=None):
        self.calls.append("lookahead0" if state is None else "lookahead")
        ops, parts = self._numpy(model, state)
        log_w, cdf, flags = contract.switching_lookahead(ops, log_prior.numpy(), parts, observation.numpy(), num_particles)
        self._flags |= flags
        return torch.from_numpy(log_w), torch.from_numpy(cdf)

    def switching_kalman_draw(self, model, state, index, uniforms, cdf, observation):
        self.calls.append("draw0" if state is None else "draw")
        ops, parts = self._numpy(model, state)
        regime, mean, cov, ell, flags = contract.switching_kalman_draw(
            ops, parts, None if index is None else index.numpy(), uniforms.numpy(), cdf.numpy(), observation.numpy())
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


def _torch_model(ops):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS])


class _Replay:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


def equal_weight_moments(want, M):
    return contract.moments(want["regimes"], want["means"], want["covariances"],
                            [np.zeros_like(w) for w in want["first_stage_log_weights"]], M)


@pytest.mark.parametrize("scheme", ["systematic", "stratified"])
def test_filter_keys_shapes_call_sequence_feeds_and_replay(backend, scheme):
    from aesmc_amd import inference, rao_blackwell
    T, B, K, M, D, Dy = 4, 3, 9, 3, 2, 2
    ops = contract.example_model(M, D, Dy, seed=5)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=3)
    gen = torch.Generator().manual_seed(1)
    regime_u = [torch.rand(B, K, dtype=torch.float64, generator=gen) for _ in range(T)]
    shape = (B, K) if scheme == "stratified" else (B,)
    resample_u = [torch.rand(shape, dtype=torch.float64, generator=gen) for _ in range(T - 1)]
    with inference.uniform_feed(_Replay(resample_u)):
        out = rao_blackwell.adapted_switching_filter(observations, model, K, resampling=scheme, regime_uniforms=regime_u,
                                                     return_moments=True, return_latents=True)
    assert sorted(out) == ["ancestral_indices", "covariances", "filtered_covariance", "filtered_mean",
                           "first_stage_log_weights", "latents", "log_marginal_likelihood", "means", "regime_probabilities",
                           "regimes"]
    assert out["log_marginal_likelihood"].shape == (B,) and out["log_marginal_likelihood"].dtype == torch.float64
    assert all(s.shape == (B, K) and s.dtype == torch.int32 for s in out["regimes"]) and len(out["regimes"]) == T
    assert all(m.shape == (B, K, D) and m.dtype == torch.float64 for m in out["means"]) and len(out["means"]) == T
    assert all(c.shape == (B, K, 3) and c.dtype == torch.float64 for c in out["covariances"]) and len(out["covariances"]) == T
    assert len(out["first_stage_log_weights"]) == T
    assert all(w.shape == (B, K) and w.dtype == torch.float64 for w in out["first_stage_log_weights"])
    assert len(out["ancestral_indices"]) == T - 1 and all(a.dtype == torch.int64 and a.shape == (B, K)
                                                          for a in out["ancestral_indices"])
    assert backend.calls == ["lookahead0", "draw0"] + ["lookahead", "resample", "draw"] * (T - 1)
    want = contract.adapted_switching_pass([y.numpy() for y in observations], ops, K, [u.numpy() for u in regime_u],
                                           [u.numpy() for u in resample_u])
    assert want["flags"] == 0
    assert min(want["margins"]["resampling"]) > 1e-9 and min(want["margins"]["regimes"]) > 1e-9
    for name in ("regimes", "ancestral_indices"):
        assert all(np.array_equal(got.numpy(), expected) for got, expected in zip(out[name], want[name]))
    for name in ("means", "covariances", "first_stage_log_weights"):
        for got, expected, tolerance in zip(out[name], want[name], want["tolerances"][name]):
            assert np.abs(got.numpy() - expected).max() <= tolerance
    assert np.abs(out["log_marginal_likelihood"].numpy() - want["log_marginal_likelihood"]).max() <= \
        want["tolerances"]["log_marginal_likelihood"]
    fm, fc, rp = equal_weight_moments(want, M)
    np.testing.assert_allclose(out["filtered_mean"].numpy(), fm, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["filtered_covariance"].numpy(), fc, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["regime_probabilities"].numpy(), rp, rtol=0, atol=1e-12)
    assert len(out["latents"]) == T and torch.equal(out["latents"][-1], out["regimes"][-1])
    lineage = np.arange(K)[None, :].repeat(B, axis=0)
    for index in reversed(want["ancestral_indices"]):
        lineage = np.take_along_axis(index, lineage, axis=1)
    assert np.array_equal(out["latents"][0].numpy(), np.take_along_axis(want["regimes"][0], lineage, axis=1))
    # a feed of the other scheme's shape
    other = [torch.rand((B,) if scheme == "stratified" else (B, K), dtype=torch.float64) for _ in range(T - 1)]
    with inference.uniform_feed(_Replay(other)), pytest.raises(ValueError, match="uniforms per step"):
        rao_blackwell.adapted_switching_filter(observations, model, K, resampling=scheme, regime_uniforms=regime_u)
    # without the switches the optional entries are absent; fresh regime uniforms come from torch's generator
    torch.manual_seed(7)
    first = rao_blackwell.adapted_switching_filter(observations, model, K, resampling="stratified")
    torch.manual_seed(7)
    again = rao_blackwell.adapted_switching_filter(observations, model, K, resampling="stratified")
    assert "latents" not in first and "filtered_mean" not in first
    assert torch.equal(first["log_marginal_likelihood"], again["log_marginal_likelihood"])


def test_refusals_and_parameter_validation(backend):
    from aesmc_amd import distributed, rao_blackwell
    ops = contract.example_model(2, 2, 1, seed=6)
    model = _torch_model(ops)
    observations = model.simulate(3, 2, seed=1)
    run = lambda **kw: rao_blackwell.adapted_switching_filter(kw.pop("observations", observations), kw.pop("model", model),
                                                              kw.pop("K", 4), **kw)
    with pytest.raises(ValueError, match="adapted_switching_filter: .*at least one timestep"):
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
        values = {name: torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS}
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


def _singular_model(rao_blackwell):
    """One regime, r = 0 and two identical rows of C: the second pivot of S is exactly 0."""
    return rao_blackwell.SwitchingLinearGaussian([1.0], [[1.0]], torch.zeros(2), 1.0, torch.eye(2)[None], torch.zeros(1, 2),
                                                 torch.ones(1, 2), torch.tensor([[[1.0, 0.0], [1.0, 0.0]]]),
                                                 torch.zeros(1, 2), torch.zeros(1, 2))


def test_a_singular_innovation_raises_and_an_exception_discards_pending_flags(backend):
    from aesmc_amd import rao_blackwell
    singular = _singular_model(rao_blackwell)
    observations = [torch.zeros(2, 2, dtype=torch.float64)] * 3
    with pytest.raises(FloatingPointError):
        rao_blackwell.adapted_switching_filter(observations, singular, 4)
    with pytest.raises(FloatingPointError):      # one step: no resampling launch to see the NaN — the end's own check
        rao_blackwell.adapted_switching_filter(observations[:1], singular, 4)
    bad = [torch.zeros(2, 4, dtype=torch.float64)] * 2 + [torch.zeros(2, 5, dtype=torch.float64)]
    with pytest.raises(ValueError, match=r"regime_uniforms\[2\]"):
        rao_blackwell.adapted_switching_filter(observations, singular, 4, regime_uniforms=bad)
    assert backend.read_flags(None) == 0
    model = _torch_model(contract.example_model(2, 2, 1, seed=6))
    out = rao_blackwell.adapted_switching_filter(model.simulate(3, 2, seed=1), model, 4)
    assert torch.isfinite(out["log_marginal_likelihood"]).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_product_filter_refuses_cpu_tensors():
    from aesmc_amd import rao_blackwell
    model = _torch_model(contract.example_model(2, 2, 1, seed=6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rao_blackwell.adapted_switching_filter(model.simulate(2, 2, seed=1), model, 4)


# ---- known answers ----------------------------------------------------------------------------------------------------------
def _pass(model, ys, K, seed, stratified=False):
    T, B = len(ys), ys[0].shape[0]
    rng = np.random.default_rng(seed)
    return contract.adapted_switching_pass(ys, model, K, [rng.uniform(size=(B, K)) for _ in range(T)],
                                           [rng.uniform(size=(B, K) if stratified else B) for _ in range(T - 1)])


@pytest.mark.parametrize("K", [1, 9])
def test_one_step_is_exact_for_any_number_of_particles(K):
    M, D, Dy, B = 3, 2, 2, 4
    model = contract.example_model(M, D, Dy, seed=8)
    y = np.random.default_rng(81).standard_normal(Dy)
    out = _pass(model, [np.broadcast_to(y, (B, Dy)).copy()], K, 82)
    _, ell = _restated_scores(model, _log(model["pi0"]), None, y[None], 1)
    want = np.log((model["pi0"] * np.exp(ell[0, 0])).sum())
    tolerance = out["tolerances"]["log_marginal_likelihood"]
    print("difference", np.abs(out["log_marginal_likelihood"] - want).max(), "tolerance", tolerance)
    assert tolerance < 1e-12
    assert (out["log_marginal_likelihood"] == out["log_marginal_likelihood"][0]).all()      # identical in every batch row
    # np.linalg's restatement is itself exact to 1e-13 here (a 2 x 2 system of condition below 1e2)
    assert np.abs(out["log_marginal_likelihood"] - want).max() <= tolerance + 1e-13
    np.testing.assert_allclose(want, contract.exact_log_likelihood(model, [y]), rtol=0, atol=1e-13)


def one_regime_case(D=3, Dy=2, seed=11):
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.standard_normal((D, D)))[0] * 0.7
    C = np.eye(Dy, D) + 0.3 * rng.standard_normal((Dy, D))
    q, r = rng.uniform(0.3, 0.8, D), rng.uniform(0.3, 0.8, Dy)
    m0, s0 = rng.standard_normal(D), rng.uniform(0.5, 1.5, D)
    return (A, C, q, r, m0, s0), rng


@pytest.mark.parametrize("K", [1, 7])
def test_one_regime_is_the_kalman_filter(K):
    T, B, D, Dy = 6, 3, 3, 2
    (A, C, q, r, m0, s0), rng = one_regime_case(D, Dy)
    model = contract.operands([1.0], [[1.0]], m0, s0, A[None], np.zeros((1, D)), q[None], C[None], np.zeros((1, Dy)), r[None])
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    out = _pass(model, ys, K, 12)
    means, covs, total = adapted_contract.kalman_filter(A, C, q, r, m0, s0, ys)
    tolerance = out["tolerances"]["log_marginal_likelihood"]
    print("difference", np.abs(out["log_marginal_likelihood"] - total).max(), "tolerance", tolerance)
    assert np.abs(out["log_marginal_likelihood"] - total).max() <= tolerance
    assert all((cdf_free == 0).all() for cdf_free in out["regimes"])
    for t in range(T):
        np.testing.assert_allclose(out["means"][t], np.broadcast_to(means[t][:, None, :], (B, K, D)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(contract.unpack(out["covariances"][t], D), np.broadcast_to(covs[t], (B, K, D, D)),
                                   rtol=0, atol=1e-12)


def shared_dynamics_case(M=3, D=3, Dy=2, seed=13):
    """M regimes that share A, b, q, C, d, r: the regimes do not matter, the model is one linear-Gaussian model."""
    (A, C, q, r, m0, s0), rng = one_regime_case(D, Dy, seed)
    Pi = rng.uniform(0.1, 1.0, (M, M))
    pi0 = rng.uniform(0.1, 1.0, M)
    model = contract.operands(pi0 / pi0.sum(), Pi / Pi.sum(axis=1, keepdims=True), m0, s0, A[None], np.zeros((1, D)), q[None],
                              C[None], np.zeros((1, Dy)), r[None])
    return model, (A, C, q, r, m0, s0), rng


@pytest.mark.parametrize("seed", [14, 15])
def test_shared_dynamics_is_the_kalman_filter_whatever_the_uniforms(seed):
    T, B, K = 6, 3, 7
    model, (A, C, q, r, m0, s0), rng = shared_dynamics_case()
    ys = [rng.standard_normal((B, 2)) for _ in range(T)]
    out = _pass(model, ys, K, seed, stratified=seed % 2 == 1)
    _, _, total = adapted_contract.kalman_filter(A, C, q, r, m0, s0, ys)
    tolerance = out["tolerances"]["log_marginal_likelihood"]
    print("difference", np.abs(out["log_marginal_likelihood"] - total).max(), "tolerance", tolerance)
    assert len(set(np.concatenate([s.ravel() for s in out["regimes"]]).tolist())) == 3      # all three regimes are drawn
    assert np.abs(out["log_marginal_likelihood"] - total).max() <= tolerance


# ---- exact zeros in the transition matrix ----------------------------------------------------------------------------------------
def left_to_right_model(singular=False):
    """Three regimes that can only stay or move one to the right; from the last there is no way back.  `singular`: regime 0
    — which nothing but regime 0 can reach — gets r = 0 and two identical rows of C, an innovation covariance of rank one."""
    M, D, Dy = 3, 2, 2
    base = contract.example_model(M, D, Dy, seed=9)
    Pi = np.array([[0.7, 0.3, 0.0], [0.0, 0.6, 0.4], [0.0, 0.0, 1.0]])
    C, r = base["C"].copy(), base["r"].copy()
    if singular:
        C[0] = np.array([[1.0, 0.0], [1.0, 0.0]])
        r[0] = 0.0
    return contract.operands([0.0, 1.0, 0.0] if singular else [0.5, 0.5, 0.0], Pi, base["m0"],
                             np.ones(D) if singular else base["s0"], base["A"], base["b"],
                             base["q"], C, base["d"], r)


@pytest.mark.parametrize("singular", [False, True])
def test_a_regime_of_prior_probability_zero_is_never_drawn_and_gives_no_nan(singular):
    model = left_to_right_model(singular)
    B, K, M, D, Dy = 2, 50, 3, 2, 2
    rng = np.random.default_rng(91)
    factor = rng.standard_normal((B, K, D, D))
    low = 1 if singular else 0      # (under `singular` no particle is in regime 0: its own row gives it a positive prior)
    state = (rng.integers(low, M, (B, K)).astype(np.int32), rng.standard_normal((B, K, D)),
             contract.pack(factor @ np.swapaxes(factor, -1, -2) / D + 0.1 * np.eye(D)))
    y = rng.standard_normal((B, Dy))
    for log_prior, given in ((_log(model["Pi"]), state), (_log(model["pi0"]), None)):
        if singular:      # (the case is what it says: K31's contract under regime 0 alone has pivots that are not positive)
            always_first = dict(model, cdf0=np.ones(M), cdf=np.ones((M, M)))
            assert np.isnan(contract.switching_kalman_step(always_first, given, None, np.zeros((B, K)), y)[3]).any()
        log_w, cdf, flags = contract.switching_lookahead(model, log_prior, given, y, K)
        bound_w, bound_c = contract.switching_lookahead_bound(model, log_prior, given, y, K)
        assert flags == 0 and np.isfinite(log_w).all() and np.isfinite(cdf).all()
        assert np.isfinite(bound_w).all() and np.isfinite(bound_c).all()
        posterior = np.diff(np.concatenate([np.zeros((B, K, 1)), cdf], axis=2), axis=2)
        prior = np.exp(log_prior)[given[0]] if given is not None else np.broadcast_to(np.exp(log_prior), (B, K, M))
        assert (posterior[prior == 0] == 0).all() and (prior == 0).any()
        np.testing.assert_allclose(posterior.sum(axis=2), 1.0, rtol=0, atol=1e-14)
        # 10^4 uniforms, the largest below 1 among them: no regime of probability zero is drawn, no NaN appears
        for chunk in range(10 ** 4 // (B * K)):
            u = rng.uniform(size=(B, K))
            if chunk == 0:
                u[0, :3] = [0.0, np.nextafter(1.0, 0.0), 0.5]
            regime, mean, cov, ell, bits = contract.switching_kalman_draw(model, given, None, u, cdf, y)
            assert bits == 0 and (prior[np.arange(B)[:, None], np.arange(K)[None, :], regime] > 0).all()
            assert np.isfinite(mean).all() and np.isfinite(cov).all() and np.isfinite(ell).all()
    # the whole filter through such a model
    T = 5
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    out = _pass(model, ys, K, 92)
    assert out["flags"] == 0 and np.isfinite(out["log_marginal_likelihood"]).all()
    for t in range(1, T):
        parents = np.take_along_axis(out["regimes"][t - 1], out["ancestral_indices"][t - 1], axis=1)
        assert (model["Pi"][parents, out["regimes"][t]] > 0).all()
    assert (model["pi0"][out["regimes"][0]] > 0).all()


def test_a_singular_innovation_under_a_positive_prior_is_nan_in_the_contract():
    model = left_to_right_model(singular=True)
    model = dict(model, pi0=np.array([0.5, 0.5, 0.0]))
    y = np.zeros((2, 2))
    log_w, cdf, flags = contract.switching_lookahead(model, _log(model["pi0"]), None, y, 4)
    assert flags == 0 and np.isnan(log_w).all() and np.isnan(cdf).all()
    bound_w, bound_c = contract.switching_lookahead_bound(model, _log(model["pi0"]), None, y, 4)
    assert (bound_w == 0).all() and (bound_c == 0).all()


def test_a_stored_regime_out_of_range_is_nan_there_only():
    model, state, _, _, y = contract.example_step(2, 65, 3, 8, 8)
    log_Pi = _log(model["Pi"])
    clean = contract.switching_lookahead(model, log_Pi, state, y)
    bad = state[0].copy()
    bad[0, 7], bad[1, 11] = 3, -1
    log_w, cdf, flags = contract.switching_lookahead(model, log_Pi, (bad, state[1], state[2]), y)
    poisoned = np.zeros((2, 65), dtype=bool)
    poisoned[0, 7] = poisoned[1, 11] = True
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE and clean[2] == 0
    assert np.isnan(log_w[poisoned]).all() and np.isnan(cdf[poisoned]).all()
    assert np.array_equal(log_w[~poisoned], clean[0][~poisoned]) and np.array_equal(cdf[~poisoned], clean[1][~poisoned])


# ---- unbiasedness and variance ------------------------------------------------------------------------------------------------------
def unbiasedness_case():
    """(model, ys [T x [R,Dy]], exact) of the unbiasedness check: ONE series, repeated as R batch rows."""
    M, D, Dy, T, R = 2, 2, 1, 4, 2000
    model = contract.example_model(M, D, Dy, seed=3)
    rng = np.random.default_rng(31)
    series = [rng.standard_normal(Dy) for _ in range(T)]
    exact = contract.exact_log_likelihood(model, series)
    return model, [np.broadcast_to(y, (R, Dy)).copy() for y in series], exact


def test_the_contract_is_unbiased():
    model, ys, exact = unbiasedness_case()
    R, K = ys[0].shape[0], 4
    out = _pass(model, ys, K, 32)
    ratio = np.exp(out["log_marginal_likelihood"] - exact)
    standard_error = ratio.std(ddof=1) / np.sqrt(R)
    print("mean", ratio.mean(), "standard error", standard_error)
    assert standard_error <= 0.01
    assert ratio.std(ddof=1) > 0      # (K = 4 particles do not make the estimate exact: there is something to average)
    assert abs(ratio.mean() - 1.0) <= 4 * standard_error


def variance_case():
    """(model, ys [T x [R,1]], K) of the variance comparison: `contract.sticky_example`, one series as R = 200 batch rows."""
    model, series = contract.sticky_example(T=12, seed=0)
    return model, [np.broadcast_to(y, (200, 1)).copy() for y in series], 8


def test_the_lookahead_has_the_smaller_variance_where_regimes_are_sticky_and_emissions_apart():
    model, ys, K = variance_case()
    T, R = len(ys), ys[0].shape[0]
    rng = np.random.default_rng(5)
    regime_u = [rng.uniform(size=(R, K)) for _ in range(T)]
    resample_u = [rng.uniform(size=R) for _ in range(T - 1)]
    adapted = contract.adapted_switching_pass(ys, model, K, regime_u, resample_u)["log_marginal_likelihood"]
    bootstrap = contract.switching_pass(ys, model, K, regime_u, resample_u)["log_marginal_likelihood"]
    assert np.isfinite(adapted).all() and np.isfinite(bootstrap).all()
    print("variance of log Z-hat: look-ahead", adapted.var(ddof=1), "bootstrap", bootstrap.var(ddof=1))
    assert adapted.var(ddof=1) < bootstrap.var(ddof=1)
    assert bootstrap.var(ddof=1) >= 2 * adapted.var(ddof=1)
