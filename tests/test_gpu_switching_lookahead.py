"""The look-ahead (fully adapted) Rao-Blackwellised filter for switching linear-Gaussian models on the device: kernels K32
(aesmc_switching_lookahead) and K33 (aesmc_switching_kalman_draw) against their NumPy contract
(aesmc_amd/testing/rao_blackwell.py) within the contract's bounds, the out-of-range and singular-innovation conventions, and
`aesmc_amd.rao_blackwell.adapted_switching_filter` end to end: replayed against the contract's pass, against the Kalman
filter where the regimes do not matter, and statistically against the exact likelihood."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as adapted_contract
from aesmc_amd.testing import rao_blackwell as contract

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
# contract.STEP_SHAPES reach the instantiations <2,2>, <4,2>, <8,2>, <8,4> and <8,8> of the padded extents; these the other four
MORE_SHAPES = [(2, 65, 2, 2, 3), (2, 65, 2, 2, 7), (2, 65, 3, 4, 4), (2, 65, 2, 3, 6)]


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device):
    return None if array is None else torch.from_numpy(np.array(array)).to(device)


def _ops(model, device):
    return {name: _dev(value, device) for name, value in model.items()}


def _device_lookahead(provider, device, model, log_prior, state, y, K):
    out = provider.switching_lookahead(_ops(model, device), _dev(log_prior, device),
                                       None if state is None else tuple(_dev(part, device) for part in state),
                                       _dev(y, device), num_particles=K)
    return [part.cpu().numpy() for part in out]


def _device_draw(provider, device, model, state, idx, uniforms, cdf, y):
    out = provider.switching_kalman_draw(_ops(model, device), None if state is None else tuple(_dev(part, device) for part in state),
                                         _dev(idx, device), _dev(uniforms, device), _dev(cdf, device), _dev(y, device))
    return [part.cpu().numpy() for part in out]


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


class _Replay:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("later", [True, False])
@pytest.mark.parametrize("B,K,M,D,Dy", contract.STEP_SHAPES + MORE_SHAPES)
def test_lookahead_equals_contract_within_the_bound(hip_device, B, K, M, D, Dy, later, observation_dtype):
    provider = _provider()
    model, state, _, _, y = contract.example_step(B, K, M, D, Dy, later=later, observation_dtype=observation_dtype)
    log_prior = _log(model["Pi"] if later else model["pi0"])
    log_w, cdf = _device_lookahead(provider, hip_device, model, log_prior, state, y, K)
    assert provider.read_flags(hip_device) == 0
    want = contract.switching_lookahead(model, log_prior, state, y, K)
    bounds = contract.switching_lookahead_bound(model, log_prior, state, y, K)
    assert log_w.shape == (B, K) and cdf.shape == (B, K, M) and log_w.dtype == np.float64 and cdf.dtype == np.float64
    assert (cdf[:, :, -1] == 1.0).all()
    for name, got, expected, bound in zip(("log_weight", "cdf"), (log_w, cdf), want[:2], bounds):
        error = np.abs(got - expected)
        print(name, "largest error", error.max(), "of bound", (error / bound).max())
        assert (error <= bound).all(), name


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("index,later", [("none", True), ("sorted", True), ("unsorted", True), ("none", False)])
@pytest.mark.parametrize("B,K,M,D,Dy", contract.STEP_SHAPES)
def test_draw_equals_contract_regimes_exact_the_rest_within_k31s_bound(hip_device, B, K, M, D, Dy, index, later,
                                                                       observation_dtype):
    provider = _provider()
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index=index, later=later,
                                                           observation_dtype=observation_dtype)
    _, cdf, _ = contract.switching_lookahead(model, _log(model["Pi"] if later else model["pi0"]), state, y, K)
    regime, mean, cov, ell = _device_draw(provider, hip_device, model, state, idx, uniforms, cdf, y)
    assert provider.read_flags(hip_device) == 0
    want = contract.switching_kalman_draw(model, state, idx, uniforms, cdf, y)
    bounds = contract.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y)
    assert regime.dtype == np.int32 and np.array_equal(regime, want[0])      # (the CDF is an input: nothing to excuse)
    assert mean.shape == (B, K, D) and cov.shape == (B, K, D * (D + 1) // 2) and ell.shape == (B, K)
    for name, got, expected, bound in zip(("mean", "cov", "log_likelihood"), (mean, cov, ell), want[1:4], bounds):
        error = np.abs(got - expected)
        print(name, "largest error", error.max(), "of bound", (error / bound).max())
        assert (error <= bound).all(), name


@pytest.mark.parametrize("B,K,M,D,Dy", [(2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_the_draws_likelihood_is_the_lookaheads_score_less_the_prior(hip_device, B, K, M, D, Dy):
    """l_s from K33 equals K32's g_s - log Pi[s', s], g_s recovered from the differences of the device's CDF row: within the
    two bounds combined."""
    provider = _provider()
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index="unsorted")
    log_Pi = _log(model["Pi"])
    log_w, cdf = _device_lookahead(provider, hip_device, model, log_Pi, state, y, K)
    regime, _, _, ell = _device_draw(provider, hip_device, model, state, idx, uniforms, cdf, y)
    assert provider.read_flags(hip_device) == 0
    bound_w, bound_c = contract.switching_lookahead_bound(model, log_Pi, state, y, K)
    bound_l = contract.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y)[2]
    rows = np.arange(B)[:, None]
    g, bound_g = contract.score_from_cdf(log_w[rows, idx], cdf[rows, idx], regime, bound_w[rows, idx], bound_c[rows, idx])
    log_prior = log_Pi[state[0][rows, idx], regime]
    error = np.abs(ell - (g - log_prior))
    bound = bound_g + bound_l + contract.UNIT * (np.abs(g) + np.abs(log_prior))
    print("largest error", error.max(), "of bound", (error / bound).max(), "largest bound", bound.max())
    assert bound.max() < 1e-6 and (error <= bound).all()


def test_draw_out_of_range_ancestor_and_regime_give_nan_there_only(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 2, 300, 4, 5, 3
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index="unsorted")
    _, cdf, _ = contract.switching_lookahead(model, _log(model["Pi"]), state, y, K)
    clean = _device_draw(provider, hip_device, model, state, idx, uniforms, cdf, y)
    assert provider.read_flags(hip_device) == 0
    bad_idx, bad_regime = idx.copy(), state[0].copy()
    bad_idx[0, 3], bad_idx[1, 299], bad_idx[1, 0] = -1, K, 1 << 40
    poisoned = np.zeros((B, K), dtype=bool)
    poisoned[0, 3] = poisoned[1, 299] = poisoned[1, 0] = True
    got = _device_draw(provider, hip_device, model, state, bad_idx, uniforms, cdf, y)
    want = contract.switching_kalman_draw(model, state, bad_idx, uniforms, cdf, y)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE == want[4]
    for part, reference, expected in zip(got, clean, want[:4]):
        assert np.array_equal(part[~poisoned], reference[~poisoned])
        assert np.array_equal(np.isnan(part.astype(np.float64)), np.isnan(expected.astype(np.float64)))
    assert np.isnan(got[1][poisoned]).all() and np.isnan(got[2][poisoned]).all() and np.isnan(got[3][poisoned]).all()
    assert (got[0][poisoned] == 0).all()
    # a stored regime outside [0, M): every particle that descends from it
    bad_regime[0, 7], bad_regime[1, 11] = M, -1
    poisoned = (idx == 7) & (np.arange(B)[:, None] == 0) | (idx == 11) & (np.arange(B)[:, None] == 1)
    assert poisoned.any()
    got = _device_draw(provider, hip_device, model, (bad_regime, state[1], state[2]), idx, uniforms, cdf, y)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    for part, reference in zip(got, clean):
        assert np.array_equal(part[~poisoned], reference[~poisoned])
    assert np.isnan(got[1][poisoned]).all() and np.isnan(got[2][poisoned]).all() and np.isnan(got[3][poisoned]).all()


def test_lookahead_stored_regime_out_of_range_gives_nan_there_only(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 2, 300, 4, 5, 3
    model, state, _, _, y = contract.example_step(B, K, M, D, Dy)
    log_Pi = _log(model["Pi"])
    clean = _device_lookahead(provider, hip_device, model, log_Pi, state, y, K)
    assert provider.read_flags(hip_device) == 0
    bad = state[0].copy()
    bad[0, 7], bad[1, 299], bad[1, 256] = M, -1, 1 << 20
    poisoned = np.zeros((B, K), dtype=bool)
    poisoned[0, 7] = poisoned[1, 299] = poisoned[1, 256] = True
    log_w, cdf = _device_lookahead(provider, hip_device, model, log_Pi, (bad, state[1], state[2]), y, K)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    assert contract.switching_lookahead(model, log_Pi, (bad, state[1], state[2]), y, K)[2] == contract.FLAG_INDEX_OUT_OF_RANGE
    assert np.isnan(log_w[poisoned]).all() and np.isnan(cdf[poisoned]).all()
    assert np.array_equal(log_w[~poisoned], clean[0][~poisoned]) and np.array_equal(cdf[~poisoned], clean[1][~poisoned])


def test_a_regime_of_prior_probability_zero_is_ignored_on_the_device(hip_device):
    """A left-to-right chain with exact zeros, the unreachable regime given a singular innovation (r = 0, two identical rows
    of C): its posterior is exactly 0, it is never drawn, nothing is NaN, no flag."""
    from tests.test_switching_lookahead_contract import left_to_right_model
    provider = _provider()
    model = left_to_right_model(singular=True)
    B, K, M, D, Dy = 2, 300, 3, 2, 2
    rng = np.random.default_rng(93)
    factor = rng.standard_normal((B, K, D, D))
    state = (rng.integers(1, M, (B, K)).astype(np.int32), rng.standard_normal((B, K, D)),
             np.ascontiguousarray(contract.pack(factor @ np.swapaxes(factor, -1, -2) / D + 0.1 * np.eye(D))))
    y = rng.standard_normal((B, Dy))
    for log_prior, given in ((_log(model["Pi"]), state), (_log(model["pi0"]), None)):
        log_w, cdf = _device_lookahead(provider, hip_device, model, log_prior, given, y, K)
        want = contract.switching_lookahead(model, log_prior, given, y, K)
        bounds = contract.switching_lookahead_bound(model, log_prior, given, y, K)
        assert np.isfinite(log_w).all() and np.isfinite(cdf).all()
        assert (np.abs(log_w - want[0]) <= bounds[0]).all() and (np.abs(cdf - want[1]) <= bounds[1]).all()
        posterior = np.diff(np.concatenate([np.zeros((B, K, 1)), cdf], axis=2), axis=2)
        prior = np.exp(log_prior)[given[0]] if given is not None else np.broadcast_to(np.exp(log_prior), (B, K, M))
        assert (posterior[prior == 0] == 0).all()
        u = rng.uniform(size=(B, K))
        u[0, :2] = [0.0, np.nextafter(1.0, 0.0)]
        regime, mean, cov, ell = _device_draw(provider, hip_device, model, given, None, u, cdf, y)
        assert (prior[np.arange(B)[:, None], np.arange(K)[None, :], regime] > 0).all()
        assert np.isfinite(mean).all() and np.isfinite(cov).all() and np.isfinite(ell).all()
    assert provider.read_flags(hip_device) == 0


def test_a_singular_innovation_under_a_positive_prior_raises_floating_point_error(hip_device):
    """r = 0 and two identical rows of C under the only regime: the second pivot is exactly 0 — the first-stage weights are
    NaN and the filter reports them at its end, for T = 3 (the resampling launch sees them) and T = 1 (nothing does)."""
    from aesmc_amd import rao_blackwell
    singular = rao_blackwell.SwitchingLinearGaussian([1.0], [[1.0]], torch.zeros(2), 1.0, torch.eye(2)[None], torch.zeros(1, 2),
                                                     torch.ones(1, 2), torch.tensor([[[1.0, 0.0], [1.0, 0.0]]]),
                                                     torch.zeros(1, 2), torch.zeros(1, 2)).to(hip_device)
    observations = [torch.zeros(2, 2, dtype=torch.float64, device=hip_device)] * 3
    with pytest.raises(FloatingPointError):
        rao_blackwell.adapted_switching_filter(observations, singular, 8)
    with pytest.raises(FloatingPointError):
        rao_blackwell.adapted_switching_filter(observations[:1], singular, 8)
    assert _provider().read_flags(hip_device) == 0


def replay_case(B, K, M, D, Dy, seed, scheme, T=6):
    """(ops, ys, regime uniforms, resampling uniforms) of the replay test; the seeds are chosen on the CPU so that the
    contract alone has every margin above 1000 x its tolerance (the test asserts it)."""
    ops = contract.example_model(M, D, Dy, seed)
    rng = np.random.default_rng([seed, 78])
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    regime_u = [rng.uniform(size=(B, K)) for _ in range(T)]
    resample_u = [rng.uniform(size=(B, K) if scheme == "stratified" else B) for _ in range(T - 1)]
    return ops, ys, regime_u, resample_u


@pytest.mark.parametrize("scheme", ["systematic", "stratified"])
@pytest.mark.parametrize("B,K,M,D,Dy,seed", [(2, 300, 4, 5, 3, 0), (2, 65, 3, 8, 8, 0)])
def test_filter_on_replayed_uniforms_equals_the_contracts_pass(hip_device, B, K, M, D, Dy, seed, scheme):
    from aesmc_amd import inference, rao_blackwell
    ops, ys, regime_u, resample_u = replay_case(B, K, M, D, Dy, seed, scheme)
    T = len(ys)
    model = _torch_model(ops, hip_device)
    with inference.uniform_feed(_Replay([_dev(u, hip_device) for u in resample_u])):
        out = rao_blackwell.adapted_switching_filter([_dev(y, hip_device) for y in ys], model, K, resampling=scheme,
                                                     regime_uniforms=[_dev(u, hip_device) for u in regime_u],
                                                     return_moments=True, return_latents=True)
    want = contract.adapted_switching_pass(ys, ops, K, regime_u, resample_u)
    tolerances = want["tolerances"]
    # no row is excused: every margin must exceed 1000 x the tolerance of what it is compared with
    for margin, tolerance in zip(want["margins"]["resampling"], tolerances["first_stage_log_weights"][1:]):
        print("resampling margin", margin, "log-weight tolerance", tolerance)
        assert margin > 1000 * tolerance
    for margin, tolerance in zip(want["margins"]["regimes"], tolerances["cdf"]):
        print("regime margin", margin, "cdf tolerance", tolerance)
        assert margin > 1000 * tolerance
    for name in ("ancestral_indices", "regimes"):
        assert len(out[name]) == len(want[name])
        assert all(np.array_equal(got.cpu().numpy(), expected) for got, expected in zip(out[name], want[name])), name
    for name in ("means", "covariances", "first_stage_log_weights"):
        assert len(out[name]) == T
        for got, expected, tolerance in zip(out[name], want[name], tolerances[name]):
            assert np.abs(got.cpu().numpy() - expected).max() <= tolerance, name
    assert np.abs(out["log_marginal_likelihood"].cpu().numpy() - want["log_marginal_likelihood"]).max() <= \
        tolerances["log_marginal_likelihood"]
    # the moments under equal weights and the genealogy, against the contract's
    fm, fc, rp = contract.moments(want["regimes"], want["means"], want["covariances"],
                                  [np.zeros((B, K))] * T, M)
    # a term moves by its system's tolerance (times 1 + 2 |m| for m m^T), the K equal-weight terms are summed in another
    # order ((K + 4) u), and the covariance subtracts mean mean^T once more
    scale = 1.0 + max(float(np.abs(m).max()) for m in want["means"]) ** 2 + max(float(np.abs(c).max()) for c in want["covariances"])
    slack = 4 * (max(tolerances["means"]) + max(tolerances["covariances"]) + (K + 4) * contract.UNIT) * scale
    print("moment slack", slack)
    np.testing.assert_allclose(out["filtered_mean"].cpu().numpy(), fm, rtol=0, atol=slack)
    np.testing.assert_allclose(out["filtered_covariance"].cpu().numpy(), fc, rtol=0, atol=slack)
    np.testing.assert_allclose(out["regime_probabilities"].cpu().numpy(), rp, rtol=0, atol=slack)
    assert len(out["latents"]) == T and torch.equal(out["latents"][-1], out["regimes"][-1])
    lineage = np.arange(K)[None, :].repeat(B, axis=0)
    for index in reversed(want["ancestral_indices"]):
        lineage = np.take_along_axis(index, lineage, axis=1)
    assert np.array_equal(out["latents"][0].cpu().numpy(), np.take_along_axis(want["regimes"][0], lineage, axis=1))


def _fresh_run(hip_device, ops, ys, K, scheme="systematic"):
    """The filter on the device with fresh uniforms of its own, and the contract's tolerance for such a pass."""
    from aesmc_amd import rao_blackwell
    T, B = len(ys), ys[0].shape[0]
    out = rao_blackwell.adapted_switching_filter([_dev(y, hip_device) for y in ys], _torch_model(ops, hip_device), K,
                                                 resampling=scheme)
    rng = np.random.default_rng(17)
    want = contract.adapted_switching_pass(ys, ops, K, [rng.uniform(size=(B, K)) for _ in range(T)],
                                           [rng.uniform(size=B) for _ in range(T - 1)])
    return out, want["tolerances"]["log_marginal_likelihood"]


@pytest.mark.parametrize("K", [1, 300])
def test_one_regime_is_the_kalman_filter_on_the_device(hip_device, K):
    from tests.test_switching_lookahead_contract import one_regime_case
    T, B, D, Dy = 6, 3, 3, 2
    (A, C, q, r, m0, s0), rng = one_regime_case(D, Dy)
    ops = contract.operands([1.0], [[1.0]], m0, s0, A[None], np.zeros((1, D)), q[None], C[None], np.zeros((1, Dy)), r[None])
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    torch.manual_seed(3)
    np.random.seed(3)
    out, tolerance = _fresh_run(hip_device, ops, ys, K)
    _, _, total = adapted_contract.kalman_filter(A, C, q, r, m0, s0, ys)
    # both are exact filters of the same model whatever the uniforms: the pass's own tolerance is the whole bound
    difference = np.abs(out["log_marginal_likelihood"].cpu().numpy() - total).max()
    print("difference", difference, "tolerance", tolerance)
    assert difference <= tolerance


@pytest.mark.parametrize("scheme", ["systematic", "stratified"])
def test_shared_dynamics_is_the_kalman_filter_on_the_device(hip_device, scheme):
    from tests.test_switching_lookahead_contract import shared_dynamics_case
    T, B, K = 6, 3, 300
    ops, (A, C, q, r, m0, s0), rng = shared_dynamics_case()
    ys = [rng.standard_normal((B, 2)) for _ in range(T)]
    torch.manual_seed(4)
    np.random.seed(4)
    out, tolerance = _fresh_run(hip_device, ops, ys, K, scheme)
    _, _, total = adapted_contract.kalman_filter(A, C, q, r, m0, s0, ys)
    difference = np.abs(out["log_marginal_likelihood"].cpu().numpy() - total).max()
    print("difference", difference, "tolerance", tolerance)
    assert len(torch.unique(torch.stack(out["regimes"]))) == 3      # (all three regimes are drawn: they do not matter)
    assert difference <= tolerance


def test_the_filter_is_unbiased_on_the_device(hip_device):
    """The mean of exp(log Z-hat - exact) over R = 2000 replicas (batch rows of one call, fresh device uniforms) against
    the contract's own: within 4 sqrt(2) standard errors of 1 and of the contract's mean, the standard error taken from
    the contract's runs."""
    from aesmc_amd import rao_blackwell
    from tests.test_switching_lookahead_contract import unbiasedness_case
    ops, ys, exact = unbiasedness_case()
    T, R, K = len(ys), ys[0].shape[0], 4
    rng = np.random.default_rng(32)
    host = contract.adapted_switching_pass(ys, ops, K, [rng.uniform(size=(R, K)) for _ in range(T)],
                                           [rng.uniform(size=R) for _ in range(T - 1)])
    host_ratio = np.exp(host["log_marginal_likelihood"] - exact)
    standard_error = host_ratio.std(ddof=1) / np.sqrt(R)
    assert 0 < standard_error <= 0.01
    torch.manual_seed(5)
    np.random.seed(5)
    for scheme in ("systematic", "stratified"):
        out = rao_blackwell.adapted_switching_filter([_dev(y, hip_device) for y in ys], _torch_model(ops, hip_device), K,
                                                     resampling=scheme)
        ratio = np.exp(out["log_marginal_likelihood"].cpu().numpy() - exact)
        print(scheme, "device mean", ratio.mean(), "contract mean", host_ratio.mean(), "standard error", standard_error)
        assert abs(ratio.mean() - 1.0) <= 4 * np.sqrt(2.0) * standard_error
        assert abs(ratio.mean() - host_ratio.mean()) <= 4 * np.sqrt(2.0) * standard_error
