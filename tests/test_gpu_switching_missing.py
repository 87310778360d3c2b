"""Missing observations and forecasts for switching linear-Gaussian models on the device: the masked kernels K39
(aesmc_switching_kalman_masked_step, in K31's, K33's and K38's forms), K40 (aesmc_switching_masked_lookahead), K41
(aesmc_switching_masked_information_step) and K42 (aesmc_switching_masked_smooth_combine) against their NumPy contract
(aesmc_amd/testing/switching_missing.py) within the contract's bounds; what stands at an unobserved position of y changing
nothing; a mask that observes everything against the unmasked entries bit for bit; `observed=` of `aesmc_amd.rao_blackwell`
end to end on replayed uniforms against the contract's masked passes; and `switching_forecast`."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_missing as missing
from tests.test_switching_missing_contract import REPLAY_SHAPES, assert_margins, replay_case

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
# of contract.STEP_SHAPES, (B, K, M, D, Dy): Dy = 1, where a mask is all or nothing; the LDS-resident P-; Dy padded 3 to 4 and a
# workgroup that straddles rows with different masks; the largest M
SHAPES = [(3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3), (1, 257, 16, 8, 1)]
assert all(shape in contract.STEP_SHAPES for shape in SHAPES)
VARIANTS = [0, 1, 2]      # `missing.example_mask`: every row is mixed, fully observed and empty once


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


def _parts(state, device):
    return None if state is None else tuple(_dev(part, device) for part in state)


def _host(out):
    return [part.cpu().numpy() for part in out]


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


class _Replay:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


def _case(B, K, M, D, Dy, variant, later=True):
    """`contract.example_step`'s inputs (float32 observations in variant 1), a mask, and y with Inf and NaN where it is False."""
    dtype = np.float32 if variant == 1 else np.float64
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index="unsorted", later=later, observation_dtype=dtype)
    mask = missing.example_mask(B, Dy, variant)
    poisoned = y.copy()
    poisoned[~mask] = np.where(np.arange((~mask).sum()) % 2 == 0, np.nan, np.inf)
    return model, state, idx, uniforms, y, poisoned, mask


def _within(names, got, want, bounds):
    for name, value, expected, bound in zip(names, got, want, bounds):
        error = np.abs(value - expected)
        print(name, "largest error", error.max(), "largest bound", bound.max())
        assert value.shape == expected.shape and np.isfinite(value).all(), name
        assert (error <= bound).all(), name


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,K,M,D,Dy", SHAPES)
def test_masked_step_equals_contract_in_all_its_forms(hip_device, B, K, M, D, Dy, variant):
    """K39 as K31 at step 0 and later, as K33 (particle_cdf) and as K38 (pinned_regime): the regimes equal, every element of
    every particle within the masked contract's bound, no flag; a row that observed nothing weighs 0 exactly."""
    provider = _provider()
    names = ("mean", "cov", "log_weight")
    for later in (False, True):
        model, state, idx, uniforms, y, poisoned, mask = _case(B, K, M, D, Dy, variant, later)
        ops, observed = _ops(model, hip_device), _dev(mask, hip_device)
        args = (_parts(state, hip_device), _dev(idx, hip_device), _dev(uniforms, hip_device))
        got = _host(provider.switching_kalman_step(ops, *args, _dev(poisoned, hip_device), observed=observed))
        want = missing.switching_kalman_step(model, state, idx, uniforms, y, mask)
        assert provider.read_flags(hip_device) == 0 == want[4]
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0])
        _within(names, got[1:], want[1:4], missing.switching_kalman_step_bound(model, state, idx, uniforms, y, mask))
        empty = ~mask.any(axis=1)
        assert (got[3][empty] == 0).all()
    log_w, cdf, flags = missing.switching_lookahead(model, _log(model["Pi"]), state, y, mask)
    assert flags == 0
    got = _host(provider.switching_kalman_draw(ops, *args, _dev(cdf, hip_device), _dev(poisoned, hip_device), observed=observed))
    want = missing.switching_kalman_draw(model, state, idx, uniforms, cdf, y, mask)
    assert provider.read_flags(hip_device) == 0 and np.array_equal(got[0], want[0])
    _within(names, got[1:], want[1:4], missing.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y, mask))
    pinned = np.random.default_rng([B, K, M, 39]).integers(0, M, B).astype(np.int32)
    got = _host(provider.switching_kalman_conditional_step(ops, *args, _dev(pinned, hip_device), _dev(poisoned, hip_device),
                                                           observed=observed))
    want = missing.switching_kalman_conditional_step(model, state, idx, uniforms, pinned, y, mask)
    assert provider.read_flags(hip_device) == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[0][:, K - 1], pinned)
    _within(names, got[1:], want[1:4],
            missing.switching_kalman_conditional_step_bound(model, state, idx, uniforms, pinned, y, mask))


@pytest.mark.parametrize("later", [True, False])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,K,M,D,Dy", SHAPES)
def test_masked_lookahead_equals_contract_within_the_bound(hip_device, B, K, M, D, Dy, variant, later):
    provider = _provider()
    model, state, _, _, y, poisoned, mask = _case(B, K, M, D, Dy, variant, later)
    log_prior = _log(model["Pi"] if later else model["pi0"])
    got = _host(provider.switching_lookahead(_ops(model, hip_device), _dev(log_prior, hip_device), _parts(state, hip_device),
                                             _dev(poisoned, hip_device), num_particles=K, observed=_dev(mask, hip_device)))
    assert provider.read_flags(hip_device) == 0
    want = missing.switching_lookahead(model, log_prior, state, y, mask, K)
    assert want[2] == 0 and (got[1][:, :, -1] == 1.0).all()
    _within(("log_weight", "cdf"), got, want[:2], missing.switching_lookahead_bound(model, log_prior, state, y, mask, K))


@pytest.mark.parametrize("steps", [1, 2])      # from the last step's zeros; from the information a masked step handed over
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,K,M,D,Dy", SHAPES)
def test_masked_information_step_equals_contract_within_the_bound(hip_device, B, K, M, D, Dy, variant, steps):
    """K41 with one trajectory per lane of the shape's K: every element of Om, lam, c and the factor F within the masked
    contract's bound.  A mask makes Om rank-deficient where the unmasked step's is not (7 of 8 components observed: rank 7),
    and the pivot of a column that is zero in exact arithmetic is rounding noise, which for some regimes of this model lies
    at the threshold 2^-40 max_i Om_ii itself (the leading block is ill-conditioned though Om's nonzero eigenvalues are
    not): the contract's bound of such a column is infinite where float64 keeps it, and extended precision drops it.  So
    the pattern of kept columns is not asserted here, only the bound — K34's rule, masked or not."""
    provider = _provider()
    model, _, _, _, y, poisoned, mask = _case(B, K, M, D, Dy, variant)
    rng = np.random.default_rng([B, K, M, D, Dy, variant, 42])
    info = None
    if steps == 2:
        before = missing.example_mask(B, Dy, (variant + 1) % 3)
        om, lam, c, _, flags, _ = missing.switching_information_step(model, rng.integers(0, M, (B, K)).astype(np.int32), None,
                                                                     rng.standard_normal((B, Dy)), before)
        info = (om, lam, c)
    regime_next = rng.integers(0, M, (B, K)).astype(np.int32)
    got = _host(provider.switching_information_step(_ops(model, hip_device), _dev(regime_next, hip_device),
                                                    _parts(info, hip_device), _dev(poisoned, hip_device),
                                                    observed=_dev(mask, hip_device)))
    assert provider.read_flags(hip_device) == 0
    want = missing.switching_information_step(model, regime_next, info, y, mask)
    assert want[4] == 0
    _within(("Om", "lam", "c", "F"), got, want[:4], missing.switching_information_step_bound(model, regime_next, info, y, mask))
    if steps == 1:      # a row that observed nothing, from the zeros: zeros, and a zero factor
        empty = ~mask.any(axis=1)
        assert not got[0][empty].any() and not got[1][empty].any() and not got[2][empty].any() and not got[3][empty].any()


def _all_entries(provider, device, model, state, idx, uniforms, y, mask, K):
    """Every masked launch on one set of inputs (mask None: the unmasked entries), as one list of tensors."""
    ops = _ops(model, device)
    keyword = {} if mask is None else {"observed": _dev(mask, device)}
    args = (_parts(state, device), _dev(idx, device), _dev(uniforms, device))
    obs = _dev(y, device)
    out = list(provider.switching_kalman_step(ops, *args, obs, **keyword))
    out += list(provider.switching_kalman_step(ops, None, None, args[2], obs, **keyword))
    look = provider.switching_lookahead(ops, _dev(_log(model["Pi"]), device), args[0], obs, num_particles=K, **keyword)
    out += list(look)
    out += list(provider.switching_lookahead(ops, _dev(_log(model["pi0"]), device), None, obs, num_particles=K, **keyword))
    out += list(provider.switching_kalman_draw(ops, *args, look[1], obs, **keyword))
    pinned = torch.zeros(y.shape[0], dtype=torch.int32, device=device)
    out += list(provider.switching_kalman_conditional_step(ops, *args, pinned, obs, **keyword))
    first = provider.switching_information_step(ops, args[0][0], None, obs, **keyword)
    out += list(first)
    second = provider.switching_information_step(ops, args[0][0], first[:3], obs, **keyword)
    out += list(second)
    seen = {} if mask is None else {"observed_next": keyword["observed"]}
    out += list(provider.switching_smooth_combine(ops, args[0][0], (args[0][1], args[0][2]), second[3], second[1], first[0],
                                                  args[0][2], **seen))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,K,M,D,Dy", SHAPES)
def test_what_stands_at_an_unobserved_position_changes_no_bit(hip_device, B, K, M, D, Dy, variant):
    """NaN and Inf at the unobserved positions of y against zeros there: every output of every masked launch bit for bit."""
    provider = _provider()
    model, state, idx, uniforms, y, poisoned, mask = _case(B, K, M, D, Dy, variant)
    zeros = np.where(mask, y, 0).astype(y.dtype)
    clean = _all_entries(provider, hip_device, model, state, idx, uniforms, zeros, mask, K)
    dirty = _all_entries(provider, hip_device, model, state, idx, uniforms, poisoned, mask, K)
    assert provider.read_flags(hip_device) == 0
    for position, (a, b) in enumerate(zip(clean, dirty)):
        assert bool(torch.isfinite(a.to(torch.float64)).all()) and torch.equal(a, b), position


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,M,D,Dy", SHAPES)
def test_a_mask_that_observes_everything_is_the_unmasked_entry_bit_for_bit(hip_device, B, K, M, D, Dy, observation_dtype):
    provider = _provider()
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index="unsorted", observation_dtype=observation_dtype)
    plain = _all_entries(provider, hip_device, model, state, idx, uniforms, y, None, K)
    masked = _all_entries(provider, hip_device, model, state, idx, uniforms, y, np.ones((B, Dy), dtype=bool), K)
    assert provider.read_flags(hip_device) == 0
    for position, (a, b) in enumerate(zip(plain, masked)):
        assert torch.equal(a, b), position


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N,M,D,Dy", [(3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_masked_combination_equals_contract_within_the_bound(hip_device, B, N, M, D, Dy, variant):
    """K42: the cross-covariance under the mask of time t+1 (the smoothed mean and covariance do not read it)."""
    provider = _provider()
    model, regime_next, filtered, factor, lam, omega_next, cov_next = contract.example_smooth_combine(B, N, M, D, Dy, steps=2)
    mask = missing.example_mask(B, Dy, variant)
    got = _host(provider.switching_smooth_combine(_ops(model, hip_device), _dev(regime_next, hip_device),
                                                  _parts(tuple(filtered), hip_device), _dev(factor, hip_device),
                                                  _dev(lam, hip_device), _dev(omega_next, hip_device), _dev(cov_next, hip_device),
                                                  observed_next=_dev(mask, hip_device)))
    assert provider.read_flags(hip_device) == 0
    args = (model, regime_next, filtered, factor, lam, omega_next, cov_next, mask)
    want = missing.switching_smooth_combine(*args)
    assert want[3] == 0
    _within(("mean", "cov", "cross"), got, want[:3], missing.switching_smooth_combine_bound(*args))
    plain = contract.switching_smooth_combine(*args[:7])
    assert mask.all() or not np.array_equal(want[2], plain[2])      # (the mask matters to the cross-covariance)


def test_the_provider_refuses_a_mask_that_is_not_bool_of_the_observations_shape_on_its_device(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 3, 7, 2, 2, 1
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy)
    ops, args, obs = _ops(model, hip_device), (_parts(state, hip_device), None, _dev(uniforms, hip_device)), _dev(y, hip_device)
    good = torch.ones((B, Dy), dtype=torch.bool, device=hip_device)
    for bad in (good.to(torch.uint8), good[:2], good.cpu(), np.ones((B, Dy), dtype=bool), good[:, :0]):
        with pytest.raises(ValueError, match="observed"):
            provider.switching_kalman_step(ops, *args, obs, observed=bad)
        with pytest.raises(ValueError, match="observed"):
            provider.switching_lookahead(ops, ops["Pi"].log(), args[0], obs, observed=bad)
        with pytest.raises(ValueError, match="observed"):
            provider.switching_information_step(ops, args[0][0], None, obs, observed=bad)
    assert provider.read_flags(hip_device) == 0


# ---- the filters on replayed uniforms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adapted", [False, True])
@pytest.mark.parametrize("scheme", ["systematic", "stratified"])
@pytest.mark.parametrize("B,K,M,D,Dy,seed", REPLAY_SHAPES)
def test_masked_filters_on_replayed_uniforms_equal_the_contracts_pass(hip_device, B, K, M, D, Dy, seed, scheme, adapted):
    """The structure of the unmasked replay tests: masks drawn with p = 0.6, step 1 row 1 fully observed, step 2 row 0 empty,
    step 3 empty in every row; Inf at the unobserved positions.  Regimes and ancestors exactly, floats and the evidence
    within the pass's tolerances; no row is excused (the margins are asserted, here and on the CPU)."""
    from aesmc_amd import inference, rao_blackwell
    ops, ys, masks, regime_u, resample_u = replay_case(B, K, M, D, Dy, seed, scheme)
    T = len(ys)
    model = _torch_model(ops, hip_device)
    run = rao_blackwell.adapted_switching_filter if adapted else rao_blackwell.switching_filter
    with inference.uniform_feed(_Replay([_dev(u, hip_device) for u in resample_u])):
        out = run([_dev(y, hip_device) for y in ys], model, K, resampling=scheme,
                  regime_uniforms=[_dev(u, hip_device) for u in regime_u], observed=[_dev(mask, hip_device) for mask in masks])
    want = (missing.adapted_switching_pass if adapted else missing.switching_pass)(ys, masks, ops, K, regime_u, resample_u)
    assert want["flags"] == 0
    assert_margins(want, adapted)
    tolerances = want["tolerances"]
    for name in ("ancestral_indices", "regimes"):
        assert len(out[name]) == len(want[name])
        assert all(np.array_equal(got.cpu().numpy(), expected) for got, expected in zip(out[name], want[name])), name
    for name in ("means", "covariances", "first_stage_log_weights" if adapted else "log_weights"):
        assert len(out[name]) == T
        for t, (got, expected, tolerance) in enumerate(zip(out[name], want[name], tolerances[name])):
            error = np.abs(got.cpu().numpy() - expected).max()
            print(name, t, "error", error, "tolerance", tolerance)
            assert error <= tolerance, (name, t)
    error = np.abs(out["log_marginal_likelihood"].cpu().numpy() - want["log_marginal_likelihood"]).max()
    print("evidence error", error, "tolerance", tolerances["log_marginal_likelihood"])
    assert error <= tolerances["log_marginal_likelihood"]
    if not adapted:
        assert not out["log_weights"][3].any()      # nothing observed: the weights say nothing, exactly


# ---- the smoothers and the conditional sweep on replayed uniforms ---------------------------------------------------------------------
SMALL = dict(T=4, B=3, K=65, N=9, M=3, D=8, Dy=8)


def _small_case(seed):
    T, B, K, N, M, D, Dy = (SMALL[name] for name in ("T", "B", "K", "N", "M", "D", "Dy"))
    ops, ys, masks, regime_u, resample_u = replay_case(B, K, M, D, Dy, seed, "systematic", T=T)
    return T, B, K, N, M, D, Dy, ops, ys, masks, regime_u, resample_u


@pytest.mark.parametrize("adapted", [False, True])
def test_masked_backward_simulation_on_replayed_uniforms_equals_the_contracts_pass(hip_device, adapted):
    """The rule of the unmasked test: the contract's backward pass runs on what the device stored; every index and regime is
    equal, except draws whose contract margin is within 4 e, e the score bounds summed along the trajectory; at most 0.1 %
    of the draws may be excused — of these 108, none."""
    from aesmc_amd import inference, rao_blackwell
    T, B, K, N, M, D, Dy, ops, ys, masks, regime_u, resample_u = _small_case(1)
    model = _torch_model(ops, hip_device)
    observations, observed = [_dev(y, hip_device) for y in ys], [_dev(mask, hip_device) for mask in masks]
    uniforms = [np.random.default_rng([7, t]).uniform(size=(B, N)) for t in range(T)]
    run = rao_blackwell.adapted_switching_filter if adapted else rao_blackwell.switching_filter
    with inference.uniform_feed(_Replay([_dev(u, hip_device) for u in resample_u])):
        filtered = run(observations, model, K, resampling="systematic", regime_uniforms=[_dev(u, hip_device) for u in regime_u],
                       observed=observed)
    out = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N,
                                                    uniforms=[_dev(u, hip_device) for u in uniforms], return_indices=True,
                                                    observed=observed)
    keys = ("regimes", "means", "covariances") + (() if adapted else ("log_weights",))
    stored = {key: [part.cpu().numpy() for part in filtered[key]] for key in keys}
    want = missing.switching_backward_pass(stored, ops, ys, masks, uniforms)
    assert want["flags"] == 0 and min(want["pivot_margins"]) > 1e-13
    excused, carried, count = np.zeros((B, N), dtype=bool), np.zeros((B, N)), 0
    for t in range(T - 1, -1, -1):
        carried = carried + want["score_bounds"][t]
        excused |= want["margins"][t] <= 4.0 * carried
        count += int(excused.sum())
        index, regime = out["indices"][t].cpu().numpy(), out["regimes"][t].cpu().numpy()
        differs = (index != want["indices"][t]) | (regime != want["regimes"][t])
        assert not (differs & ~excused).any(), t
        excused |= differs
    print("excused draws", count, "of", T * B * N, "smallest margin", min(float(m.min()) for m in want["margins"]))
    assert count <= 0.001 * T * B * N


def _norms(error_means, error_covs, D):
    return (float(np.linalg.norm(error_means, axis=-1).max()),
            float(np.linalg.norm(contract.unpack(error_covs, D), 2, axis=(-2, -1)).max()))


def test_masked_state_smoother_along_given_regimes_equals_the_contracts_pass(hip_device):
    """`conditional_kalman_filter` and `switching_state_smooth` under the masks against the masked `switching_state_pass`
    within the tolerances it propagates, the cross-covariances (K42) included."""
    from aesmc_amd import rao_blackwell
    T, B, K, N, M, D, Dy, ops, ys, masks, _, _ = _small_case(2)
    model = _torch_model(ops, hip_device)
    observations, observed = [_dev(y, hip_device) for y in ys], [_dev(mask, hip_device) for mask in masks]
    rng = np.random.default_rng(9)
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    paths = [_dev(regime, hip_device) for regime in regimes]
    want = missing.switching_state_pass(ops, regimes, ys, masks)
    tolerances = want["tolerances"]
    assert want["flags"] == 0 and min(want["pivot_margins"]) > 1e-13
    filtered = rao_blackwell.conditional_kalman_filter(observations, model, paths, observed=observed)
    out = rao_blackwell.switching_state_smooth(observations, model, paths, return_cross_moments=True, return_trajectories=True,
                                               observed=observed)
    for result in (filtered, out):
        assert np.abs(result["log_likelihood"].cpu().numpy() - want["log_likelihood"]).max() <= tolerances["log_likelihood"]
    for t in range(T):
        error_m, error_p = _norms(filtered["means"][t].cpu().numpy() - want["filtered_means"][t],
                                  filtered["covariances"][t].cpu().numpy() - want["filtered_covariances"][t], D)
        assert error_m <= tolerances["filtered_means"][t] and error_p <= tolerances["filtered_covariances"][t], t
        error_m, error_p = _norms(out["means"][t].cpu().numpy() - want["means"][t],
                                  out["covariances"][t].cpu().numpy() - want["covariances"][t], D)
        assert error_m <= tolerances["means"][t] and error_p <= tolerances["covariances"][t], t
        if t < T - 1:
            error_x = float(np.linalg.norm(out["cross_covariances"][t].cpu().numpy() - want["cross_covariances"][t], 2,
                                           axis=(-2, -1)).max())
            print("cross", t, "error", error_x, "tolerance", tolerances["cross_covariances"][t])
            assert error_x <= tolerances["cross_covariances"][t], t


@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_a_masked_sweep_on_replayed_uniforms_equals_the_contracts_pass(hip_device, ancestor_sampling):
    """The rule of the unmasked sweep's test (tests/test_gpu_switching_gibbs.py), rows excused as there; of these draws none
    may be (0.1 % of 588 is less than one)."""
    from aesmc_amd import rao_blackwell
    T, B, K, N, M, D, Dy, ops, ys, masks, regime_u, _ = _small_case(3)
    model = _torch_model(ops, hip_device)
    rng = np.random.default_rng([3, 37])
    reference = [rng.integers(0, M, B).astype(np.int32) for _ in range(T)]
    uniforms = [rng.uniform(size=(B, K)) for _ in range(T - 1)] + [rng.uniform(size=(B, 1))]
    dev = lambda blocks: [_dev(block, hip_device) for block in blocks]
    path, particles = rao_blackwell.conditional_switching_filter(
        dev(ys), model, K, dev(reference), ancestor_sampling=ancestor_sampling, uniforms=dev(uniforms),
        regime_uniforms=dev(regime_u), return_particles=True, observed=dev(masks))
    want = missing.conditional_switching_pass(ys, masks, ops, K, reference, uniforms, regime_u,
                                              ancestor_sampling=ancestor_sampling)
    assert want["flags"] == 0
    rounding = 8 * K * contract.UNIT
    excused, count = np.zeros(B, dtype=bool), 0
    for t in range(T):
        if t > 0:
            carried = want["tolerances"]["log_weights"][t - 1] + rounding
            margins = want["margins"][t - 1]
            free = margins[:, :K - 1] <= 4.0 * carried
            pinned = margins[:, K - 1] <= 4.0 * (carried + want["score_bounds"][t - 1])
            count += int(free.sum() + pinned.sum())
            excused |= free.any(axis=1) | pinned
            differs = (particles["ancestral_indices"][t - 1].cpu().numpy() != want["ancestral_indices"][t - 1]).any(axis=1)
            assert not (differs & ~excused).any(), t
            excused |= differs
        regime = particles["regimes"][t].cpu().numpy()
        assert np.array_equal(regime[:, K - 1], reference[t])
        differs = (regime != want["regimes"][t]).any(axis=1)
        assert not (differs & ~excused).any(), t
        excused |= differs
        keep = ~excused
        mean_error = np.linalg.norm(particles["means"][t].cpu().numpy() - want["means"][t], axis=-1)[keep]
        cov_error = np.linalg.norm(contract.unpack(particles["covariances"][t].cpu().numpy() - want["covariances"][t], D), 2,
                                   axis=(-2, -1))[keep]
        weight_error = np.abs(particles["log_weights"][t].cpu().numpy() - want["log_weights"][t])[keep]
        assert (mean_error <= want["tolerances"]["means"][t]).all(), t
        assert (cov_error <= want["tolerances"]["covariances"][t]).all(), t
        assert (weight_error <= want["tolerances"]["log_weights"][t]).all(), t
    last = want["margins"][T - 1] <= 4.0 * (want["tolerances"]["log_weights"][T - 1] + rounding)
    count += int(last.sum())
    excused |= last
    for t in range(T):
        keep = ~excused
        assert np.array_equal(particles["indices"][t].cpu().numpy()[keep], want["indices"][t][keep]), t
        assert np.array_equal(path[t].cpu().numpy()[keep], want["path"][t][keep]), t
    draws = (T - 1) * B * K + B
    print("excused draws", count, "of", draws)
    assert count <= 0.001 * draws


# ---- the forecast ----------------------------------------------------------------------------------------------------------------------
def test_the_forecast_of_one_regime_is_the_closed_form(hip_device):
    """M = 1: h steps ahead the state is N(A^h m + sum_{i<h} A^i b, A^h P A^hT + sum_{i<h} A^i Q A^iT) from the filter's last
    N(m, P), the observation C of it plus d and R — by np.linalg.  Tolerance: the forecast's steps are predictions, whose
    bound the masked contract gives per step (composed as `switching_pass` composes a pass's: the tolerance of H steps from
    an exact start) plus the rounding of the restatement, (H D + 4) u on sums of terms of the sizes involved; the filter's
    last system enters both sides as the device wrote it."""
    from aesmc_amd import rao_blackwell
    from tests.test_switching_lookahead_contract import one_regime_case
    T, H, B, D, Dy, K = 5, 4, 3, 3, 2, 1
    (A, C, q, r, m0, s0), rng = one_regime_case(D, Dy)
    b, d = 0.3 * rng.standard_normal(D), 0.3 * rng.standard_normal(Dy)
    ops = contract.operands([1.0], [[1.0]], m0, s0, A[None], b[None], q[None], C[None], d[None], r[None])
    model = _torch_model(ops, hip_device)
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    filtered = rao_blackwell.switching_filter([_dev(y, hip_device) for y in ys], model, K, resampling="systematic")
    out = rao_blackwell.switching_forecast(filtered, model, H)
    assert _provider().read_flags(hip_device) == 0
    assert torch.equal(out["log_weight"], filtered["log_weights"][-1])
    mean = filtered["means"][-1].cpu().numpy()[:, 0]
    cov = contract.unpack(filtered["covariances"][-1].cpu().numpy()[:, 0], D)
    state = tuple(filtered[key][-1].cpu().numpy() for key in ("regimes", "means", "covariances"))
    nothing = np.zeros((B, Dy), dtype=bool)
    tolerance = 0.0
    for h in range(H):
        mean, cov = mean @ A.T + b, A @ cov @ A.T + np.diag(q ** 2)
        bound_m, bound_p, _ = missing.switching_kalman_step_bound(ops, state, None, np.zeros((B, K)), np.zeros((B, Dy)), nothing)
        state = missing.switching_kalman_step(ops, state, None, np.zeros((B, K)), np.zeros((B, Dy)), nothing)[:3]
        size = 1.0 + np.abs(mean).max() ** 2 + np.abs(cov).max()
        # (|A| < 1: an earlier step's error does not grow; the observation's moments multiply it by |C|^2 at most)
        tolerance += float(bound_m.max() + bound_p.max()) + (H * D + 4) * contract.UNIT * size * D
        reach = tolerance * (1.0 + np.linalg.norm(C, 2)) ** 2 * (1.0 + 2 * np.abs(mean).max())
        print("step", h, "tolerance", tolerance, "observation's", reach)
        np.testing.assert_allclose(out["means"][h].cpu().numpy()[:, 0], mean, rtol=0, atol=tolerance)
        np.testing.assert_allclose(contract.unpack(out["covariances"][h].cpu().numpy()[:, 0], D), cov, rtol=0, atol=tolerance)
        np.testing.assert_allclose(out["state_mean"][h].cpu().numpy(), mean, rtol=0, atol=tolerance)
        np.testing.assert_allclose(out["state_covariance"][h].cpu().numpy(), cov, rtol=0, atol=reach)
        np.testing.assert_allclose(out["observation_mean"][h].cpu().numpy(), mean @ C.T + d, rtol=0, atol=reach)
        np.testing.assert_allclose(out["observation_covariance"][h].cpu().numpy(), C @ cov @ C.T + np.diag(r ** 2), rtol=0,
                                   atol=reach)
        assert (out["regime_probabilities"][h] == 1).all() and (out["regimes"][h] == 0).all()
    assert tolerance < 1e-12


@pytest.mark.parametrize("adapted", [False, True])
def test_the_forecast_of_three_regimes_is_the_contracts_masked_steps_composed(hip_device, adapted):
    """M = 3: the forecast's systems against K39's contract under an all-False mask, composed step by step here on what the
    device stored last — regimes equal (they are drawn from the model's own cumulative rows: nothing to excuse), means and
    covariances within the steps' bounds carried forward by `switching_pass`'s recurrences (tol_P = 1.01 pp tol_P + fresh,
    tol_m = 1.01 (mm tol_m + mp tol_P) + fresh, with `_sensitivities`' factors of the prediction) — and its moments against
    `contract.moments` with `switching_filter`'s slack."""
    from aesmc_amd import rao_blackwell
    T, H, B, K, M, D, Dy = 4, 5, 3, 300, 3, 5, 3
    ops = contract.example_model(M, D, Dy, seed=2)
    model = _torch_model(ops, hip_device)
    rng = np.random.default_rng(23)
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    draws = [rng.uniform(size=(B, K)) for _ in range(H)]
    run = rao_blackwell.adapted_switching_filter if adapted else rao_blackwell.switching_filter
    torch.manual_seed(6)
    np.random.seed(6)
    filtered = run([_dev(y, hip_device) for y in ys], model, K, resampling="systematic")
    out = rao_blackwell.switching_forecast(filtered, model, H, regime_uniforms=[_dev(u, hip_device) for u in draws])
    assert _provider().read_flags(hip_device) == 0
    log_w = filtered["log_weights"][-1].cpu().numpy() if not adapted else np.zeros((B, K))
    assert np.array_equal(out["log_weight"].cpu().numpy(), log_w)
    state = tuple(filtered[key][-1].cpu().numpy() for key in ("regimes", "means", "covariances"))
    nothing, blank = np.zeros((B, Dy), dtype=bool), np.zeros((B, Dy))
    systems, tol_m, tol_p = [], 0.0, 0.0
    for h in range(H):
        regime, mean, cov, zero, flags = missing.switching_kalman_step(ops, state, None, draws[h], blank, nothing)
        bound_m, bound_p, _ = missing.switching_kalman_step_bound(ops, state, None, draws[h], blank, nothing)
        pp, mm, mp, _, _ = missing._sensitivities(ops, state, None, regime, missing.mark(blank, nothing))
        fresh_m = float(np.sqrt((bound_m ** 2).sum(axis=-1)).max())
        fresh_p = float(np.sqrt((contract.unpack(bound_p, D) ** 2).sum(axis=(-2, -1))).max())
        tol_m, tol_p = 1.01 * (mm * tol_m + mp * tol_p) + fresh_m, 1.01 * pp * tol_p + fresh_p
        assert flags == 0 and not zero.any()
        assert np.array_equal(out["regimes"][h].cpu().numpy(), regime)
        error_m, error_p = _norms(out["means"][h].cpu().numpy() - mean, out["covariances"][h].cpu().numpy() - cov, D)
        print("step", h, "errors", error_m, error_p, "tolerances", tol_m, tol_p)
        assert error_m <= tol_m and error_p <= tol_p
        state = (regime, mean, cov)
        systems.append(state)
    fm, fc, rp = contract.moments(*zip(*systems), [log_w] * H, M)
    scale = 1.0 + max(float(np.abs(s[1]).max()) for s in systems) ** 2 + max(float(np.abs(s[2]).max()) for s in systems)
    slack = 4 * (tol_m + tol_p + (K + 4) * contract.UNIT) * scale
    np.testing.assert_allclose(out["state_mean"].cpu().numpy(), fm, rtol=0, atol=slack)
    np.testing.assert_allclose(out["state_covariance"].cpu().numpy(), fc, rtol=0, atol=slack)
    np.testing.assert_allclose(out["regime_probabilities"].cpu().numpy(), rp, rtol=0, atol=slack)
    # the observation's mixture, restated on the contract's systems: the same slack through |C| and |C|^2
    w = np.exp(log_w - log_w.max(axis=1, keepdims=True))
    w = w / w.sum(axis=1, keepdims=True)
    reach = slack * (1.0 + np.abs(ops["C"]).sum(axis=-1).max()) ** 2
    for h, (regime, mean, cov) in enumerate(systems):
        C, d, r = ops["C"][regime], ops["d"][regime], ops["r"][regime]
        center = np.einsum("bkil,bkl->bki", C, mean) + d
        spread = C @ contract.unpack(cov, D) @ np.swapaxes(C, -1, -2) + np.einsum("bki,ij->bkij", r ** 2, np.eye(Dy))
        average = (w[:, :, None] * center).sum(axis=1)
        second = (w[:, :, None, None] * (spread + center[:, :, :, None] * center[:, :, None, :])).sum(axis=1)
        np.testing.assert_allclose(out["observation_mean"][h].cpu().numpy(), average, rtol=0, atol=reach)
        np.testing.assert_allclose(out["observation_covariance"][h].cpu().numpy(),
                                   second - average[:, :, None] * average[:, None, :], rtol=0, atol=reach)
    assert out["observation_mean"].shape == (H, B, Dy) and out["observation_covariance"].shape == (H, B, Dy, Dy)
