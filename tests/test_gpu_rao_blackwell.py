"""The Rao-Blackwellised particle filter for switching linear-Gaussian models on the device: kernel K31
(aesmc_switching_kalman_step) against its NumPy contract (aesmc_amd/testing/rao_blackwell.py) within the contract's bound,
the out-of-range and singular-innovation conventions, and `aesmc_amd.rao_blackwell.switching_filter` end to end: replayed
against the contract's pass, against the Kalman filter for one regime, and statistically against the exact likelihood."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as adapted_contract
from aesmc_amd.testing import rao_blackwell as contract

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device):
    return None if array is None else torch.from_numpy(np.array(array)).to(device)


def _device_step(provider, device, model, state, idx, uniforms, y):
    ops = {name: _dev(value, device) for name, value in model.items()}
    out = provider.switching_kalman_step(ops, None if state is None else tuple(_dev(part, device) for part in state),
                                         _dev(idx, device), _dev(uniforms, device), _dev(y, device))
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
@pytest.mark.parametrize("index,later", [("none", True), ("sorted", True), ("unsorted", True), ("none", False)])
@pytest.mark.parametrize("B,K,M,D,Dy", contract.STEP_SHAPES)
def test_step_equals_contract_within_the_bound(hip_device, B, K, M, D, Dy, index, later, observation_dtype):
    provider = _provider()
    args = contract.example_step(B, K, M, D, Dy, index=index, later=later, observation_dtype=observation_dtype)
    regime, mean, cov, log_w = _device_step(provider, hip_device, *args)
    assert provider.read_flags(hip_device) == 0
    want = contract.switching_kalman_step(*args)
    bounds = contract.switching_kalman_step_bound(*args)
    assert regime.dtype == np.int32 and np.array_equal(regime, want[0])
    assert mean.shape == (B, K, D) and cov.shape == (B, K, D * (D + 1) // 2) and log_w.shape == (B, K)
    for name, got, expected, bound in zip(("mean", "cov", "log_weight"), (mean, cov, log_w), want[1:4], bounds):
        error = np.abs(got - expected)
        print(name, "largest error", error.max(), "of bound", (error / bound).max())
        assert (error <= bound).all(), name


def test_out_of_range_ancestor_and_regime_give_nan_there_only(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 2, 300, 4, 5, 3
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index="unsorted")
    clean = _device_step(provider, hip_device, model, state, idx, uniforms, y)
    assert provider.read_flags(hip_device) == 0
    bad_idx, bad_regime = idx.copy(), state[0].copy()
    bad_idx[0, 3], bad_idx[1, 299], bad_idx[1, 0] = -1, K, 1 << 40
    poisoned = np.zeros((B, K), dtype=bool)
    poisoned[0, 3] = poisoned[1, 299] = poisoned[1, 0] = True
    got = _device_step(provider, hip_device, model, state, bad_idx, uniforms, y)
    want = contract.switching_kalman_step(model, state, bad_idx, uniforms, y)
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
    got = _device_step(provider, hip_device, model, (bad_regime, state[1], state[2]), idx, uniforms, y)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    for part, reference in zip(got, clean):
        assert np.array_equal(part[~poisoned], reference[~poisoned])
    assert np.isnan(got[1][poisoned]).all() and np.isnan(got[2][poisoned]).all() and np.isnan(got[3][poisoned]).all()


def test_a_singular_innovation_covariance_raises_floating_point_error(hip_device):
    """r = 0 and two identical rows of C: S = C P- C^T has rank one, its second pivot is exactly 0 — an invalid value, not
    a fault: the log-weights are NaN and the filter reports them at its end."""
    from aesmc_amd import rao_blackwell
    singular = rao_blackwell.SwitchingLinearGaussian([1.0], [[1.0]], torch.zeros(2), 1.0, torch.eye(2)[None], torch.zeros(1, 2),
                                                     torch.ones(1, 2), torch.tensor([[[1.0, 0.0], [1.0, 0.0]]]),
                                                     torch.zeros(1, 2), torch.zeros(1, 2)).to(hip_device)
    observations = [torch.zeros(2, 2, dtype=torch.float64, device=hip_device)] * 3
    with pytest.raises(FloatingPointError):
        rao_blackwell.switching_filter(observations, singular, 8)
    with pytest.raises(FloatingPointError):
        rao_blackwell.switching_filter(observations[:1], singular, 8)
    assert _provider().read_flags(hip_device) == 0


@pytest.mark.parametrize("scheme", ["systematic", "stratified"])
@pytest.mark.parametrize("B,K,M,D,Dy,seed", [(2, 300, 4, 5, 3, 0), (2, 65, 3, 8, 8, 0)])
def test_filter_on_replayed_uniforms_equals_the_contracts_pass(hip_device, B, K, M, D, Dy, seed, scheme):
    from aesmc_amd import inference, rao_blackwell
    T = 6
    ops = contract.example_model(M, D, Dy, seed)
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=seed + 1)
    rng = np.random.default_rng([seed, 77])
    regime_u = [rng.uniform(size=(B, K)) for _ in range(T)]
    resample_u = [rng.uniform(size=(B, K) if scheme == "stratified" else B) for _ in range(T - 1)]
    with inference.uniform_feed(_Replay([_dev(u, hip_device) for u in resample_u])):
        out = rao_blackwell.switching_filter(observations, model, K, resampling=scheme,
                                             regime_uniforms=[_dev(u, hip_device) for u in regime_u],
                                             return_moments=True, return_latents=True)
    want = contract.switching_pass([y.cpu().numpy() for y in observations], ops, K, regime_u, resample_u)
    # no row is excused: every step's margin must exceed 1000 x the propagated log-weight tolerance
    for margin, tolerance in zip(want["margins"], want["tolerances"]["log_weights"]):
        print("margin", margin, "log-weight tolerance", tolerance)
        assert margin > 1000 * tolerance
    for name in ("ancestral_indices", "regimes"):
        assert len(out[name]) == len(want[name])
        assert all(np.array_equal(got.cpu().numpy(), expected) for got, expected in zip(out[name], want[name])), name
    for name in ("means", "covariances", "log_weights"):
        for got, expected, tolerance in zip(out[name], want[name], want["tolerances"][name]):
            assert np.abs(got.cpu().numpy() - expected).max() <= tolerance, name
    assert np.abs(out["log_marginal_likelihood"].cpu().numpy() - want["log_marginal_likelihood"]).max() <= \
        want["tolerances"]["log_marginal_likelihood"]
    # the moments and the genealogy, against the contract's
    fm, fc, rp = contract.moments(want["regimes"], want["means"], want["covariances"], want["log_weights"], M)
    assert out["filtered_mean"].shape == (T, B, D) and out["filtered_covariance"].shape == (T, B, D, D)
    assert out["regime_probabilities"].shape == (T, B, M)
    # a weight w_k = softmax(log w)_k moves by at most 2 tol_lw w_k, a term by its system's tolerance (times 1 + 2 |m| for
    # m m^T), the K terms are summed in another order ((K + 4) u), and the covariance subtracts mean mean^T once more
    tolerances = want["tolerances"]
    scale = 1.0 + max(float(np.abs(m).max()) for m in want["means"]) ** 2 + max(float(np.abs(c).max()) for c in want["covariances"])
    slack = 4 * (max(tolerances["log_weights"]) + max(tolerances["means"]) + max(tolerances["covariances"]) +
                 (K + 4) * contract.UNIT) * scale
    print("moment slack", slack)
    np.testing.assert_allclose(out["filtered_mean"].cpu().numpy(), fm, rtol=0, atol=slack)
    np.testing.assert_allclose(out["filtered_covariance"].cpu().numpy(), fc, rtol=0, atol=slack)
    np.testing.assert_allclose(out["regime_probabilities"].cpu().numpy(), rp, rtol=0, atol=slack)
    assert len(out["latents"]) == T and torch.equal(out["latents"][-1], out["regimes"][-1])
    lineage = np.arange(K)[None, :].repeat(B, axis=0)
    for index in reversed(want["ancestral_indices"]):
        lineage = np.take_along_axis(index, lineage, axis=1)
    assert np.array_equal(out["latents"][0].cpu().numpy(), np.take_along_axis(want["regimes"][0], lineage, axis=1))


@pytest.mark.parametrize("K", [1, 300])
def test_one_regime_is_the_kalman_filter_on_the_device(hip_device, K):
    from aesmc_amd import rao_blackwell
    T, B, D, Dy = 6, 3, 3, 2
    rng = np.random.default_rng(11)
    A = np.linalg.qr(rng.standard_normal((D, D)))[0] * 0.7
    C = np.eye(Dy, D) + 0.3 * rng.standard_normal((Dy, D))
    q, r = rng.uniform(0.3, 0.8, D), rng.uniform(0.3, 0.8, Dy)
    m0, s0 = rng.standard_normal(D), rng.uniform(0.5, 1.5, D)
    ops = contract.operands([1.0], [[1.0]], m0, s0, A[None], np.zeros((1, D)), q[None], C[None], np.zeros((1, Dy)), r[None])
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=5)
    ys = [y.cpu().numpy() for y in observations]
    regime_u = [rng.uniform(size=(B, K)) for _ in range(T)]
    np.random.seed(3)
    out = rao_blackwell.switching_filter(observations, model, K, resampling="systematic",
                                         regime_uniforms=[_dev(u, hip_device) for u in regime_u])
    np.random.seed(3)
    want = contract.switching_pass(ys, ops, K, regime_u, [np.random.uniform(size=[B, 1]).reshape(-1) for _ in range(T - 1)])
    _, _, total = adapted_contract.kalman_filter(A, C, q, r, m0, s0, ys)
    # both are exact filters of the same model: the pass's own tolerance is the whole bound
    tolerance = want["tolerances"]["log_marginal_likelihood"]
    assert np.abs(out["log_marginal_likelihood"].cpu().numpy() - total).max() <= tolerance
    log_p, means, covs = rao_blackwell.kalman_log_likelihood(observations, model)
    assert np.abs(log_p.cpu().numpy() - total).max() <= tolerance
    assert means.shape == (T, B, D) and covs.shape == (T, B, D, D)


def test_the_filter_is_unbiased_on_the_device(hip_device):
    """The mean of exp(log Z-hat - exact) over R = 2000 replicas (batch rows of one call, fresh device uniforms) against
    the contract's own: within 4 standard errors of the two means combined, the standard error taken from the contract's
    runs."""
    from aesmc_amd import rao_blackwell
    M, D, Dy, T, R, K = 2, 2, 1, 4, 2000, 16
    ops = contract.example_model(M, D, Dy, seed=3)
    rng = np.random.default_rng(31)
    series = [rng.standard_normal(Dy) for _ in range(T)]
    exact = contract.exact_log_likelihood(ops, series)
    ys = [np.broadcast_to(y, (R, Dy)).copy() for y in series]
    rng = np.random.default_rng(32)
    host = contract.switching_pass(ys, ops, K, [rng.uniform(size=(R, K)) for _ in range(T)],
                                   [rng.uniform(size=R) for _ in range(T - 1)])
    host_ratio = np.exp(host["log_marginal_likelihood"] - exact)
    standard_error = host_ratio.std(ddof=1) / np.sqrt(R)
    assert standard_error <= 0.01
    torch.manual_seed(5)
    np.random.seed(5)
    for scheme in ("systematic", "stratified"):
        out = rao_blackwell.switching_filter([_dev(y, hip_device) for y in ys], _torch_model(ops, hip_device), K,
                                             resampling=scheme)
        ratio = np.exp(out["log_marginal_likelihood"].cpu().numpy() - exact)
        print(scheme, "device mean", ratio.mean(), "contract mean", host_ratio.mean(), "standard error", standard_error)
        assert abs(ratio.mean() - 1.0) <= 4 * np.sqrt(2.0) * standard_error
        assert abs(ratio.mean() - host_ratio.mean()) <= 4 * np.sqrt(2.0) * standard_error
