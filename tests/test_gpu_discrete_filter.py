"""The discrete particle filter (Fearnhead & Clifford 2003) for switching linear-Gaussian models on the device: kernels K43
(aesmc_switching_lookahead_scores) and K44 (aesmc_switching_optimal_resample) against their NumPy contract
(aesmc_amd/testing/discrete_filter.py; the margins of every fixed input here are asserted in
tests/test_discrete_filter_contract.py), the bad-row conventions and statuses, and
`aesmc_amd.rao_blackwell.discrete_switching_filter` end to end: replayed against the contract's pass, against the exact
likelihood where nothing is discarded, statistically where something is, under a mask, and through the smoother and the
forecast that take its output."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import discrete_filter as contract
from aesmc_amd.testing import rao_blackwell as rb
from aesmc_amd.testing import switching_missing as missing

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


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


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


def _resample(provider, device, log_w, scores, u, K_out):
    out = provider.switching_optimal_resample(_dev(log_w, device), _dev(scores, device), _dev(u, device), K_out)
    return [part.cpu().numpy() for part in out]


# ---- K44 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", contract.RESAMPLE_PROFILES)
@pytest.mark.parametrize("B,K_in,M,K_out", contract.RESAMPLE_SHAPES)
def test_optimal_resample_equals_contract(hip_device, B, K_in, M, K_out, profile):
    provider = _provider()
    log_w, scores, u = contract.example_resample(B, K_in, M, K_out, profile)
    parent, regime, log_weight, lse, count = _resample(provider, hip_device, log_w, scores, u, K_out)
    assert provider.read_flags(hip_device) == 0
    want = contract.optimal_resample(log_w, scores, u, K_out)
    bound = want[8]
    assert parent.dtype == np.int64 and regime.dtype == np.int32 and count.dtype == np.int32
    assert np.array_equal(parent, want[0]) and np.array_equal(regime, want[1]) and np.array_equal(count, want[4])
    assert np.array_equal(np.isneginf(log_weight), np.isneginf(want[2]))
    finite = np.isfinite(want[2])
    error = np.where(finite, np.abs(log_weight - np.where(finite, want[2], 0.0)), 0.0)
    print("log_weight error over bound", (error / bound[:, None]).max(), "lse", (np.abs(lse - want[3]) / bound).max())
    assert (error <= bound[:, None]).all() and (np.abs(lse - want[3]) <= bound).all()


def test_optimal_resample_without_log_weights_is_zeros(hip_device):
    provider = _provider()
    _, scores, u = contract.example_resample(2, 65, 3, 65, "normal")
    got = _resample(provider, hip_device, None, scores, u, 65)
    zeros = _resample(provider, hip_device, np.zeros((2, 65)), scores, u, 65)
    assert provider.read_flags(hip_device) == 0
    assert all(np.array_equal(a, b) for a, b in zip(got, zeros))


def test_position_sweep_the_heavy_candidate_comes_out_first(hip_device):
    """One heavy candidate at every position i in turn (one batch row each): slot 0 carries its own parent and regime."""
    provider = _provider()
    log_w, scores, u = contract.example_sweep()
    parent, regime, log_weight, lse, count = _resample(provider, hip_device, log_w, scores, u, 4)
    assert provider.read_flags(hip_device) == 0
    want = contract.optimal_resample(log_w, scores, u, 4)
    assert np.array_equal(parent[:, 0] * 3 + regime[:, 0], np.arange(195))
    assert np.array_equal(parent, want[0]) and np.array_equal(regime, want[1]) and (count == 4).all()
    assert (np.abs(log_weight - want[2]) <= want[8][:, None]).all()


def test_a_nan_candidate_marks_its_row_alone(hip_device):
    provider = _provider()
    log_w, scores, u = contract.example_resample(3, 7, 2, 7, "normal")
    scores[1, 3, 1] = np.nan
    parent, regime, log_weight, lse, count = _resample(provider, hip_device, log_w, scores, u, 7)
    want = contract.optimal_resample(log_w, scores, u, 7)
    assert provider.read_flags(hip_device) == contract.FLAG_NAN_LOG_WEIGHT == want[5]
    assert (parent[1] == 7).all() and np.isnan(log_weight[1]).all() and np.isnan(lse[1]) and count[1] == 0
    assert np.array_equal(parent, want[0]) and np.array_equal(count, want[4]) and np.isfinite(lse[[0, 2]]).all()


def test_a_row_of_minus_infinity_is_degenerate(hip_device):
    provider = _provider()
    log_w, scores, u = contract.example_resample(2, 65, 3, 65, "normal")
    scores[0] = -np.inf
    parent, regime, log_weight, lse, count = _resample(provider, hip_device, log_w, scores, u, 65)
    assert provider.read_flags(hip_device) == contract.FLAG_DEGENERATE_ROW
    assert (parent[0] == 65).all() and np.isnan(log_weight[0]).all() and np.isnan(lse[0]) and count[0] == 0
    assert (parent[1] < 65).all() and count[1] == 65


def test_statuses(hip_device):
    from aesmc_amd import _lib
    provider = _provider()
    lib = _lib.load()
    cap = int(lib.aesmc_switching_optimal_resample_max_candidates())
    assert cap == contract.MAX_CANDIDATES == provider.switching_optimal_resample_max_candidates()
    B, K_in, M, K_out = 2, 8, 3, 8
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=hip_device)
    log_w, scores, u = f64(B, K_in), f64(B, K_in, M), f64(B) + 0.5
    parent = torch.zeros((B, K_out), dtype=torch.int64, device=hip_device)
    regime = torch.zeros((B, K_out), dtype=torch.int32, device=hip_device)
    log_weight, lse = f64(B, K_out), f64(B)
    count = torch.zeros(B, dtype=torch.int32, device=hip_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(log_w=log_w, scores=scores, u=u, parent=p(parent), regime=p(regime), log_weight=p(log_weight), lse=p(lse),
             count=p(count), B=B, K_in=K_in, M=M, K_out=K_out):
        return lib.aesmc_switching_optimal_resample(p(log_w), p(scores), p(u), parent, regime, log_weight, lse, count, None, B,
                                                    K_in, M, K_out, None)

    ok, invalid, unsupported = 0, 1, _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert call() == ok
    assert call(K_in=cap // M + 1) == unsupported and call(M=17) == unsupported      # (checked before any launch)
    assert call(log_weight=p(lse)) == invalid and call(parent=p(scores)) == invalid and call(lse=p(u)) == invalid
    assert call(regime=ctypes.c_void_p(regime.data_ptr() + 2)) == invalid
    assert call(lse=ctypes.c_void_p(lse.data_ptr() + 4)) == invalid and call(parent=None) == invalid
    assert call(B=-1) == invalid and call(M=0) == invalid
    assert call(B=0) == ok and call(K_out=0) == ok and call(K_in=0) == ok
    torch.cuda.synchronize()
    empty = provider.switching_optimal_resample(log_w[:0], scores[:0], u[:0], K_out)
    assert empty[0].shape == (0, K_out) and provider.read_flags(hip_device) == 0


def test_too_many_candidates_is_refused_naming_the_covered_class(hip_device):
    from aesmc_amd import rao_blackwell
    ops = rb.example_model(16, 2, 1)
    model = _torch_model(ops, hip_device)
    y = [torch.zeros((1, 1), dtype=torch.float64, device=hip_device)]
    with pytest.raises(NotImplementedError, match="covered: switching linear-Gaussian models"):
        rao_blackwell.discrete_switching_filter(y, model, contract.MAX_CANDIDATES // 16 + 1)


# ---- K43 --------------------------------------------------------------------------------------------------------------------
def _device_scores(provider, device, model, log_prior, state, y, K, observed=None):
    out = provider.switching_lookahead_scores(_ops(model, device), _dev(log_prior, device),
                                              None if state is None else tuple(_dev(part, device) for part in state),
                                              _dev(y, device), num_particles=K, observed=_dev(observed, device))
    return out


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("later", [True, False])
@pytest.mark.parametrize("B,K,M,D,Dy", rb.STEP_SHAPES)
def test_scores_equal_contract_and_the_lookaheads_log_weight_bitwise(hip_device, B, K, M, D, Dy, later, observation_dtype):
    provider = _provider()
    model, state, _, _, y = rb.example_step(B, K, M, D, Dy, later=later, observation_dtype=observation_dtype)
    prior = model["Pi"].copy() if later else model["pi0"].copy()
    if M > 1:      # a regime of probability zero: its score is -inf and stays
        prior[..., 0] = 0.0
        prior /= prior.sum(axis=-1, keepdims=True)
    log_prior = _log(prior)
    scores, log_weight = _device_scores(provider, hip_device, model, log_prior, state, y, K)
    device_state = None if state is None else tuple(_dev(part, hip_device) for part in state)
    k32, _ = provider.switching_lookahead(_ops(model, hip_device), _dev(log_prior, hip_device), device_state, _dev(y, hip_device),
                                          num_particles=K)
    assert provider.read_flags(hip_device) == 0
    assert torch.equal(log_weight, k32)      # the same chains in the same order
    scores = scores.cpu().numpy()
    want, _, _ = contract.switching_lookahead_scores(model, log_prior, state, y, K)
    bound, _ = contract.switching_lookahead_scores_bound(model, log_prior, state, y, K)
    assert scores.shape == (B, K, M) and np.array_equal(np.isneginf(scores), np.isneginf(want))
    if M > 1:
        assert np.isneginf(scores[:, :, 0]).all()
    finite = np.isfinite(want)
    error = np.where(finite, np.abs(scores - np.where(finite, want, 0.0)), 0.0)
    print("largest error", error.max(), "of bound", (error[finite] / bound[finite]).max())
    assert np.isfinite(scores[finite]).all() and (error <= bound).all()


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("B,K,M,D,Dy", [(3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_masked_scores_are_the_reduced_models(hip_device, B, K, M, D, Dy, variant):
    provider = _provider()
    model, state, _, _, y = rb.example_step(B, K, M, D, Dy)
    observed = missing.example_mask(B, Dy, variant)
    y = np.where(observed, y, np.nan)      # (never read where nothing was observed)
    log_prior = _log(model["Pi"])
    scores, log_weight = _device_scores(provider, hip_device, model, log_prior, state, y, K, observed=observed)
    k40, _ = provider.switching_lookahead(_ops(model, hip_device), _dev(log_prior, hip_device),
                                          tuple(_dev(part, hip_device) for part in state), _dev(y, hip_device),
                                          num_particles=K, observed=_dev(observed, hip_device))
    assert provider.read_flags(hip_device) == 0 and torch.equal(log_weight, k40)
    want, _, _ = contract.switching_lookahead_scores(model, log_prior, state, np.where(observed, y, 0.0), K, observed=observed)
    bound, _ = contract.switching_lookahead_scores_bound(model, log_prior, state, np.where(observed, y, 0.0), K,
                                                         observed=observed)
    error = np.abs(scores.cpu().numpy() - want)
    print("largest error", error.max(), "of bound", (error / bound).max())
    assert (error <= bound).all()


def test_scores_out_of_range_regime_and_singular_innovation(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 2, 65, 3, 2, 2
    model, state, _, _, y = rb.example_step(B, K, M, D, Dy)
    regime = state[0].copy()
    regime[1, 7] = M
    scores, log_weight = _device_scores(provider, hip_device, model, _log(model["Pi"]), (regime,) + state[1:], y, K)
    assert provider.read_flags(hip_device) == rb.FLAG_INDEX_OUT_OF_RANGE
    scores = scores.cpu().numpy()
    assert np.isnan(scores[1, 7]).all() and np.isnan(log_weight.cpu().numpy()[1, 7]) and np.isfinite(np.delete(scores[1], 7, 0)).all()
    singular = dict(model, r=model["r"].copy(), C=model["C"].copy())
    singular["r"][1] = 0.0
    singular["C"][1] = 0.0      # regime 1 observes nothing and has no noise: its pivots are zero
    want, _, _ = contract.switching_lookahead_scores(singular, _log(model["Pi"]), state, y, K)
    scores, log_weight = _device_scores(provider, hip_device, singular, _log(model["Pi"]), state, y, K)
    assert provider.read_flags(hip_device) == 0      # (the resampling that follows raises the flag)
    scores = scores.cpu().numpy()
    assert np.isnan(want[:, :, 1]).all() and np.array_equal(np.isnan(scores), np.isnan(want))
    assert np.isnan(log_weight.cpu().numpy()).all()


# ---- the filter -----------------------------------------------------------------------------------------------------------------
def _run(device, ops, ys, K, us=None, observed=None, **more):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.discrete_switching_filter(
        [_dev(y, device) for y in ys], _torch_model(ops, device), K, uniforms=None if us is None else [_dev(u, device) for u in us],
        observed=None if observed is None else [_dev(o, device) for o in observed], **more)


def _compare(out, want, K):
    D = want["means"][0].shape[-1]
    tolerances = want["tolerances"]
    worst = 0.0
    for t in range(len(want["regimes"])):
        assert np.array_equal(out["regimes"][t].cpu().numpy(), want["regimes"][t]), t
        assert np.array_equal(out["num_live"][t].cpu().numpy(), want["num_live"][t]), t
        if t > 0:
            assert np.array_equal(out["ancestral_indices"][t - 1].cpu().numpy(), want["ancestral_indices"][t - 1]), t
        error_m = np.linalg.norm(out["means"][t].cpu().numpy() - want["means"][t], axis=-1).max()
        error_p = np.linalg.norm(rb.unpack(out["covariances"][t].cpu().numpy() - want["covariances"][t], D), 2,
                                 axis=(-2, -1)).max()
        got_w, want_w = out["log_weights"][t].cpu().numpy(), want["log_weights"][t]
        assert np.array_equal(np.isneginf(got_w), np.isneginf(want_w))
        live = np.isfinite(want_w)
        error_w = np.abs(got_w[live] - want_w[live]).max()
        worst = max(worst, error_m / tolerances["means"][t], error_p / tolerances["covariances"][t],
                    error_w / tolerances["log_weights"][t])
        assert error_m <= tolerances["means"][t] and error_p <= tolerances["covariances"][t], t
        assert error_w <= tolerances["log_weights"][t], t
    error_z = np.abs(out["log_marginal_likelihood"].cpu().numpy() - want["log_marginal_likelihood"]).max()
    print("largest error over propagated tolerance", max(worst, error_z / tolerances["log_marginal_likelihood"]))
    assert error_z <= tolerances["log_marginal_likelihood"]
    assert torch.equal(out["log_weight"], out["log_weights"][-1])


@pytest.mark.parametrize("B,K,M,D,Dy,T", contract.FILTER_SHAPES)
def test_filter_replays_the_contracts_pass(hip_device, B, K, M, D, Dy, T):
    ops, ys, us = contract.example_series(B, M, D, Dy, T)
    want = contract.discrete_switching_pass(ys, ops, K, us)
    out = _run(hip_device, ops, ys, K, us, return_moments=True)
    assert want["flags"] == 0
    _compare(out, want, K)
    fm, fc, rp = rb.moments(want["regimes"], want["means"], want["covariances"], want["log_weights"], M)
    assert np.abs(out["filtered_mean"].cpu().numpy() - fm).max() < 1e-9
    assert np.abs(out["regime_probabilities"].cpu().numpy() - rp).max() < 1e-9


@pytest.mark.parametrize("M,D,Dy,T,K", contract.EXACT_SHAPES)
def test_filter_is_exact_while_nothing_is_discarded(hip_device, M, D, Dy, T, K):
    ops, ys, us = contract.example_series(2, M, D, Dy, T, seed=1)
    want = contract.discrete_switching_pass(ys, ops, K, us)
    out = _run(hip_device, ops, ys, K, us)
    error = np.abs(out["log_marginal_likelihood"].cpu().numpy() - rb.exact_log_likelihood(ops, ys)).max()
    print("error", error, "tolerance", want["tolerances"]["log_marginal_likelihood"])
    assert error <= 2 * want["tolerances"]["log_marginal_likelihood"]      # (the device's and the contract's, each within it)
    assert [int(c.min()) for c in out["num_live"]] == [min(M ** (t + 1), K) for t in range(T)]


def test_no_two_live_slots_share_a_genealogy(hip_device):
    B, K, M, D, Dy, T = contract.FILTER_SHAPES[0]
    ops, ys, us = contract.example_series(B, M, D, Dy, T)
    out = _run(hip_device, ops, ys, K, us, return_latents=True)
    paths = torch.stack(list(out["latents"])).cpu().numpy()      # [T,B,K]
    assert paths.shape == (T, B, K)
    for b in range(B):
        live = np.isfinite(out["log_weight"][b].cpu().numpy())
        histories = [tuple(paths[:, b, k]) for k in np.flatnonzero(live)]
        assert live.sum() == K and len(set(histories)) == len(histories)


def test_evidence_is_unbiased_where_candidates_are_discarded(hip_device):
    """B = 4096 copies of one series, fresh uniforms, K = 4 < M^T = 64: the mean of exp(log Z - exact) within 4 of its
    standard errors of 1."""
    M, T, K, B = 2, 6, 4, 4096
    ops, ys, _ = contract.example_series(1, M, 2, 1, T, seed=3)
    exact = rb.exact_log_likelihood(ops, ys)[0]
    torch.manual_seed(11)
    out = _run(hip_device, ops, [np.broadcast_to(y, (B, 1)).copy() for y in ys], K)
    ratio = np.exp(out["log_marginal_likelihood"].cpu().numpy() - exact)
    standard_error = ratio.std(ddof=1) / np.sqrt(B)
    print("mean ratio", ratio.mean(), "standard error", standard_error)
    assert standard_error > 0 and abs(ratio.mean() - 1.0) <= 4 * standard_error
    assert all((c == K).all() for c in out["num_live"][2:])


def test_constant_mask_is_the_reduced_model_and_a_nan_where_unobserved_is_harmless(hip_device):
    B, K, M, D, Dy, T = contract.FILTER_SHAPES[1]
    ops, ys, us = contract.example_series(B, M, D, Dy, T)
    keep = np.arange(Dy) % 2 == 0
    observed = [np.tile(keep, (B, 1))] * T
    want = contract.discrete_switching_pass(ys, ops, K, us, observed=observed)
    out = _run(hip_device, ops, [np.where(keep, y, np.nan) for y in ys], K, us, observed=observed)
    _compare(out, want, K)
    reduced = _run(hip_device, missing.reduced(ops, np.flatnonzero(keep)), [y[:, keep] for y in ys], K, us)
    for t in range(T):
        assert torch.equal(out["regimes"][t], reduced["regimes"][t])
    difference = (out["log_marginal_likelihood"] - reduced["log_marginal_likelihood"]).abs().max().item()
    assert difference <= 2 * want["tolerances"]["log_marginal_likelihood"]


def test_output_with_dead_slots_goes_through_the_smoother_and_the_forecast(hip_device):
    """(M, D, Dy, T, K) = (2, 2, 1, 4, 16): 2, 4 and 8 live slots of 16 at t = 0, 1, 2, the rest dead (log-weight -inf, slot
    0's state).  The filter is exact here, so the N = 4096 backward trajectories are draws from the exact smoothing
    distribution: their frequencies within 4 binomial standard errors of `exact_regime_marginals`."""
    from aesmc_amd import rao_blackwell
    M, D, Dy, T, K = contract.EXACT_SHAPES[0]
    N = 4096
    ops, ys, us = contract.example_series(1, M, D, Dy, T, seed=1)
    model = _torch_model(ops, hip_device)
    observations = [_dev(y, hip_device) for y in ys]
    filtered = rao_blackwell.discrete_switching_filter(observations, model, K, uniforms=[_dev(u, hip_device) for u in us])
    assert [int(c) for c in filtered["num_live"]] == [2, 4, 8, 16]
    assert torch.isneginf(filtered["log_weights"][0][:, 2:]).all()
    torch.manual_seed(5)
    smoothed = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N)
    got = smoothed["smoothed_regime_probabilities"].cpu().numpy()[:, 0]
    exact = rb.exact_regime_marginals(ops, [y[0] for y in ys])
    standard_error = np.sqrt(exact * (1.0 - exact) / N)
    print("largest error in standard errors", (np.abs(got - exact) / standard_error).max())
    assert (np.abs(got - exact) <= 4 * standard_error).all()
    state = rao_blackwell.switching_state_smooth(observations, model, smoothed["regimes"])      # (the trajectories drawn from it)
    assert torch.isfinite(state["smoothed_mean"]).all() and torch.isfinite(state["smoothed_covariance"]).all()
    forecast = rao_blackwell.switching_forecast(filtered, model, 2)
    for name in ("state_mean", "state_covariance", "observation_mean", "observation_covariance", "regime_probabilities"):
        assert torch.isfinite(forecast[name]).all(), name
    assert (forecast["regime_probabilities"].sum(dim=-1) - 1.0).abs().max().item() < 1e-12
