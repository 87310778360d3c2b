"""The collapsed-mixture filter and smoother of switching linear-Gaussian models on the device: kernels K50
(aesmc_switching_collapse) and K51 (aesmc_switching_pair_smooth) against their NumPy contracts
(aesmc_amd/testing/switching_collapsed.py) within the contracts' bounds, their conventions, bit-equal repeats, and
`aesmc_amd.rao_blackwell.collapsed_switching_filter` / `collapsed_switching_smooth` end to end against the contract passes
and, where the methods are exact, against the enumerations.

Pivots near a threshold: every K51 case asserts from the contract alone that each pivot lies further from its threshold than
4 times its running bound (`clearance` > 1), so that both sides keep and drop the same rows."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_collapsed as collapsed
from aesmc_amd.testing import switching_missing as missing
from tests.test_switching_collapsed_contract import (SMALL, check_special_collapse, close, degenerate_pair_inputs,
                                                     excluded_regime_model, series, shared_model, special_collapse_inputs)

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
PASS = 1e-10      # times (1 + |value|): the project's tolerance of a whole float64 pass against its contract


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device):
    return None if array is None else torch.from_numpy(np.array(array)).to(device)


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


def _device_collapse(provider, device, mean, cov, lw):
    return tuple(part.cpu().numpy() for part in provider.switching_collapse(_dev(mean, device), _dev(cov, device), _dev(lw, device)))


def _device_pair(provider, device, model, mean, cov, mean_next, cov_next):
    ops = {name: _dev(value, device) for name, value in model.items()}
    out = provider.switching_pair_smooth(ops, *[_dev(part, device) for part in (mean, cov, mean_next, cov_next)])
    return tuple(part.cpu().numpy() for part in out)


# ---- K50 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,G,N,D", collapsed.COLLAPSE_SHAPES)
def test_the_collapse_equals_the_contract_within_its_bound(hip_device, B, G, N, D, shared):
    provider = _provider()
    mean, cov, lw = collapsed.example_collapse(B, G, N, D)
    if shared:
        mean, cov = np.ascontiguousarray(mean[:, 0]), np.ascontiguousarray(cov[:, 0])
    want = collapsed.switching_collapse(mean, cov, lw)
    bounds = collapsed.switching_collapse_bound(mean, cov, lw)
    got = _device_collapse(provider, hip_device, mean, cov, lw)
    again = _device_collapse(provider, hip_device, mean, cov, lw)
    for name, value, repeat, reference, bound in zip(("log_mass", "mean", "cov"), got, again, want, bounds):
        assert value.shape == reference.shape and value.dtype == np.float64, name
        error = np.abs(value - reference)
        print(name, "largest error", error.max(), "of its bound", (error / np.maximum(bound, 1e-300)).max())
        assert (error <= bound).all(), name
        assert np.array_equal(value, repeat), name      # no atomics: the same bits


def test_the_collapses_conventions_on_the_device(hip_device):
    provider = _provider()
    mean, cov, lw = special_collapse_inputs()
    got = _device_collapse(provider, hip_device, mean, cov, lw)
    mass, centre, spread, without = check_special_collapse(*got)
    bounds = collapsed.switching_collapse_bound(mean[1:2, 0:1, [0, 1, 3]], cov[1:2, 0:1, [0, 1, 3]], lw[1:2, 0:1, [0, 1, 3]])
    assert abs(mass - without[0][0, 0]) <= bounds[0][0, 0]
    assert (np.abs(centre - without[1][0, 0]) <= bounds[1][0, 0]).all() and (np.abs(spread - without[2][0, 0]) <= bounds[2][0, 0]).all()
    want = collapsed.switching_collapse(mean, cov, lw)
    full = collapsed.switching_collapse_bound(mean, cov, lw)
    for value, reference, bound in zip(got, want, full):
        with np.errstate(invalid="ignore"):      # (the empty group's mass is -inf on both sides)
            same = np.isnan(reference) | (value == reference) | (np.abs(value - reference) <= bound)
        assert np.array_equal(np.isnan(value), np.isnan(reference)) and same.all()


# ---- K51 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,Dy", collapsed.PAIR_SHAPES)
def test_the_pair_step_equals_the_contract_within_its_bound(hip_device, B, M, D, Dy):
    provider = _provider()
    args = collapsed.example_pair_smooth(B, M, D, Dy)
    want_means, want_covs, margin = collapsed.switching_pair_smooth(*args)
    bound_m, bound_c, clearance = collapsed.switching_pair_smooth_bound(*args)
    assert clearance > 1 and margin > 0
    means, covs = _device_pair(provider, hip_device, *args)
    again = _device_pair(provider, hip_device, *args)
    assert means.shape == (B, M, M, D) and covs.shape == (B, M, M, D * (D + 1) // 2) and means.dtype == covs.dtype == np.float64
    for name, value, reference, bound in (("means", means, want_means, bound_m), ("covs", covs, want_covs, bound_c)):
        error = np.abs(value - reference)
        print(name, "largest error", error.max(), "of its bound", (error / np.maximum(bound, 1e-300)).max())
        assert (error <= bound).all(), name
    assert np.array_equal(means, again[0]) and np.array_equal(covs, again[1])


@pytest.mark.parametrize("variant", ["q1", "q", "P", "both"])
def test_degenerate_pair_steps_on_the_device(hip_device, variant):
    provider = _provider()
    args = degenerate_pair_inputs(variant)
    want_means, want_covs, _ = collapsed.switching_pair_smooth(*args)
    bound_m, bound_c, clearance = collapsed.switching_pair_smooth_bound(*args)
    assert clearance > 1
    means, covs = _device_pair(provider, hip_device, *args)
    assert np.isfinite(means).all() and np.isfinite(covs).all()
    assert (np.abs(means - want_means) <= bound_m).all() and (np.abs(covs - want_covs) <= bound_c).all()
    if variant in ("P", "both"):
        assert np.array_equal(means, np.broadcast_to(args[1][:, :, None], means.shape)) and (covs == 0).all()


# ---- whole passes ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes():
    """The contract passes of the whole-pass tests, computed once: (M, D, Dy, dtype name) -> (model, series, {what: pass})."""
    out = {}
    for M, D, Dy in [(2, 2, 1), (3, 8, 8), (4, 5, 3)]:
        model = contract.example_model(M, D, Dy)
        for dtype in (np.float32, np.float64):
            ys = [y.astype(dtype) for y in series(model, 6, 3)]
            out[M, D, Dy, np.dtype(dtype).name] = (model, ys, {
                1: collapsed.collapsed_pass(ys, model, order=1), 2: collapsed.collapsed_pass(ys, model, order=2),
                "smooth": collapsed.collapsed_smooth_pass(ys, model)})
    return out


FILTER_KEYS = ("log_marginal_likelihood", "regime_probabilities", "filtered_mean", "filtered_covariance")
SMOOTH_KEYS = ("smoothed_regime_probabilities", "smoothed_pair_probabilities", "smoothed_mean", "smoothed_covariance")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("M,D,Dy", [(2, 2, 1), (3, 8, 8), (4, 5, 3)])
def test_the_functions_equal_the_contract_passes(hip_device, passes, M, D, Dy, dtype):
    from aesmc_amd import rao_blackwell
    provider = _provider()
    model, ys, want = passes[M, D, Dy, dtype]
    slg = _torch_model(model, hip_device)
    observations = [_dev(y, hip_device) for y in ys]
    assert observations[0].dtype == getattr(torch, dtype)
    for order in (1, 2):
        out = rao_blackwell.collapsed_switching_filter(observations, slg, order=order, return_components=True)
        for key in FILTER_KEYS:
            assert close(out[key].cpu().numpy(), want[order][key], PASS), (order, key)
        for key in ("log_regime_probabilities", "means", "covariances"):
            assert all(close(got.cpu().numpy(), wanted, PASS) for got, wanted in zip(out[key], want[order][key])), (order, key)
    out = rao_blackwell.collapsed_switching_smooth(observations, slg)
    assert want["smooth"]["margin"] > 1e-6
    for key in FILTER_KEYS + SMOOTH_KEYS:
        assert close(out[key].cpu().numpy(), want["smooth"][key], PASS), key
    assert provider.read_flags(hip_device) == 0
    again = rao_blackwell.collapsed_switching_smooth(observations, slg)
    assert all(torch.equal(out[key], again[key]) for key in out)      # deterministic: the same bits


def test_a_pass_under_a_mask(hip_device):
    from aesmc_amd import rao_blackwell
    M, D, Dy, T, B = 3, 3, 2, 6, 3
    model = contract.example_model(M, D, Dy)
    ys = series(model, T, B)
    masks = missing.example_masks(T, B, Dy, seed=2)
    observed = [None if t == 2 else masks[t] for t in range(T)]
    want = collapsed.collapsed_smooth_pass(ys, model, observed=observed)
    hidden = [y if o is None else np.where(o, y, np.nan) for y, o in zip(ys, observed)]
    out = rao_blackwell.collapsed_switching_smooth([_dev(y, hip_device) for y in hidden], _torch_model(model, hip_device),
                                                   observed=[_dev(o, hip_device) for o in observed])
    for key in FILTER_KEYS + SMOOTH_KEYS:
        assert close(out[key].cpu().numpy(), want[key], PASS), key
    order_one = rao_blackwell.collapsed_switching_filter([_dev(y, hip_device) for y in hidden], _torch_model(model, hip_device),
                                                         order=1, observed=[_dev(o, hip_device) for o in observed])
    assert close(order_one["log_marginal_likelihood"].cpu().numpy(),
                 collapsed.collapsed_pass(ys, model, order=1, observed=observed)["log_marginal_likelihood"], PASS)


# ---- the exactness cases on the device ----------------------------------------------------------------------------------------------
EXACT = 1e-12


@pytest.mark.parametrize("M,D,Dy", SMALL)
def test_exact_evidence_and_regime_marginals_on_the_device(hip_device, M, D, Dy):
    from aesmc_amd import rao_blackwell
    model = contract.example_model(M, D, Dy)
    slg = _torch_model(model, hip_device)
    for T in (1, 2):
        ys = series(model, T, 3)
        observations = [_dev(y, hip_device) for y in ys]
        exact = contract.exact_log_likelihood(model, ys)
        out = rao_blackwell.collapsed_switching_filter(observations, slg, order=2)
        assert close(out["log_marginal_likelihood"].cpu().numpy(), exact, EXACT), T
        if T == 1:
            one = rao_blackwell.collapsed_switching_filter(observations, slg, order=1)
            assert close(one["log_marginal_likelihood"].cpu().numpy(), exact, EXACT)
    smooth = rao_blackwell.collapsed_switching_smooth(observations, slg)["smoothed_regime_probabilities"].cpu().numpy()
    for b in range(3):
        assert close(smooth[:, b], contract.exact_regime_marginals(model, [y[b] for y in ys]), EXACT), b


@pytest.mark.parametrize("case", ["one regime", "shared"])
def test_exact_with_one_regime_and_shared_dynamics_on_the_device(hip_device, case):
    from aesmc_amd import rao_blackwell
    model = contract.example_model(1, 3, 2) if case == "one regime" else shared_model(2, 3, 2)
    slg = _torch_model(model, hip_device)
    ys = series(model, 6, 2)
    observations = [_dev(y, hip_device) for y in ys]
    exact = contract.exact_log_likelihood(model, ys)
    for order in (1, 2):
        out = rao_blackwell.collapsed_switching_filter(observations, slg, order=order)
        assert close(out["log_marginal_likelihood"].cpu().numpy(), exact, EXACT), order
    ys = series(model, 5, 2)
    out = rao_blackwell.collapsed_switching_smooth([_dev(y, hip_device) for y in ys], slg)
    for b in range(2):
        mean, cov, _ = contract.exact_smoothed_state(model, [y[b] for y in ys])
        assert close(out["smoothed_mean"][:, b].cpu().numpy(), mean, EXACT)
        assert close(out["smoothed_covariance"][:, b].cpu().numpy(), cov, EXACT)


def test_exact_zeros_in_the_chain_on_the_device(hip_device):
    """An impossible regime with a singular innovation: K31's NaN under it reaches no score, K50 reads no dead component."""
    from aesmc_amd import rao_blackwell
    model = excluded_regime_model()
    slg = _torch_model(model, hip_device)
    ys = series(model, 4, 2)
    observations = [_dev(y, hip_device) for y in ys]
    for order in (1, 2):
        out = rao_blackwell.collapsed_switching_filter(observations, slg, order=order)
        want = collapsed.collapsed_pass(ys, model, order=order)
        assert all(bool(torch.isfinite(out[key]).all()) for key in FILTER_KEYS)
        assert all(close(out[key].cpu().numpy(), want[key], PASS) for key in FILTER_KEYS)
    out = rao_blackwell.collapsed_switching_smooth(observations, slg)
    want = collapsed.collapsed_smooth_pass(ys, model)
    assert all(bool(torch.isfinite(out[key]).all()) for key in SMOOTH_KEYS)
    assert all(close(out[key].cpu().numpy(), want[key], PASS) for key in SMOOTH_KEYS)
    assert bool((out["smoothed_regime_probabilities"][:, :, 2] == 0).all())
