"""CPU checks of the switching-model EM statistics (aesmc_amd/testing/switching_statistics.py: the contract of K45 / K46 and
of `switching_expected_statistics`, `switching_m_step`, `switching_score`): the contract's pass against brute-force loops,
Fisher's identity against autograd through a dense Kalman filter, stationarity of the M-step, exact EM with one regime,
shared parameters, the host logic of `aesmc_amd.rao_blackwell` on a provider double, and the status codes of the three C
entries."""
import numpy as np
import pytest
import torch

from aesmc_amd import _lib
from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_missing as missing
from aesmc_amd.testing import switching_statistics as stats
from tests.oracle_provider import OracleKernels

NAMES = ("transition_counts", "next_next", "next_prev", "prev_prev", "obs_obs", "obs_state", "state_state", "initial_counts",
         "initial_state")
MODEL_KEYS = stats.PARAMETERS
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="non-empty sizes on made-up pointers: only where nothing can launch")


def _masks(T, B, Dy, seed=0):
    """T bool [B,Dy] masks: components observed with probability 0.6, row 0 of step 0 unobserved, the last step (T >= 2)
    unobserved altogether."""
    rng = np.random.default_rng([seed, T, B, Dy, 46])
    masks = [rng.uniform(size=(B, Dy)) < 0.6 for _ in range(T)]
    masks[0][0] = False
    if T >= 2:
        masks[-1][:] = False
    return masks


def _poisoned(observations, masks):
    out = []
    for y, mask in zip(observations, masks):
        y = y.copy()
        y[~mask] = np.nan
        out.append(y)
    return out


# ---- 1. the contract's pass against the brute-force loops ------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 1), (2, 4, 3), (2, 3, 5), (16, 8, 8)], ids=str)
def test_pass_against_brute_force(shape, T, masked):
    (M, D, Dy), B, N = shape, 2, 3
    smoothed, observations = stats.example_smoothed(B, N, M, D, Dy, T)
    masks = _masks(T, B, Dy) if masked else None
    if masked:
        observations = _poisoned(observations, masks)
    got = stats.expected_statistics(smoothed, observations, M, masks)
    want = stats.brute_force_statistics(smoothed, observations, M, masks)
    assert got["flags"] == 0 and (got["batch_size"], got["num_trajectories"], got["num_timesteps"]) == (B, N, T)
    for name in NAMES:
        error = np.abs(got[name] - want[name])
        assert got[name].shape == want[name].shape and np.isfinite(got[name]).all(), name
        assert (error <= 2.0 * got["bounds"][name]).all(), (name, float(error.max()))
    assert got["initial_counts"].sum() == B * N and got["transition_counts"].sum() == (T - 1) * B * N
    if T > 1 and D > 1:      # the orientation: rows of a cross-covariance at the later time
        turned = dict(smoothed, cross_covariances=[np.swapaxes(x, -1, -2) for x in smoothed["cross_covariances"]])
        wrong = stats.expected_statistics(turned, observations, M, masks)
        assert (np.abs(wrong["next_prev"] - want["next_prev"]) > 2.0 * got["bounds"]["next_prev"]).any()


def test_step_layout_and_out_of_range():
    B, N, M, D, Dy = 2, 9, 3, 2, 2
    y, regime, mean, cov, previous = stats.example_step(B, N, M, D, Dy)
    where = stats.layout(D, Dy, True)
    assert where["columns"] == 6 + 2 + 6 + 12 + 16 + 3 + 6 + 6 and stats.layout(D, Dy, False)["columns"] == where["columns"] - 12
    clean, magnitude, flags = stats.statistics_step(y, regime, mean, cov, M, previous)
    assert flags == 0 and (clean[M:] == 0).all() and (magnitude >= np.abs(clean)).all()
    assert clean[:, stats.layout(D, Dy, False)["counts"]].sum() == B * N
    initial, _, _ = stats.statistics_step(y, regime, mean, cov, M)
    assert (initial[:, stats.layout(D, Dy, False)["counts"].start:] == 0).all()
    bad = regime.copy()
    bad[1, 4] = M
    without, _, flags = stats.statistics_step(y, bad, mean, cov, M, previous)
    assert flags == stats.FLAG_INDEX_OUT_OF_RANGE
    alone, _, _ = stats.statistics_step(y[1:], regime[1:, 4:5], mean[1:, 4:5], cov[1:, 4:5], M,
                                        tuple(part[1:, 4:5] for part in previous))
    assert np.abs(clean - alone - without).max() <= 2.0 * stats.statistics_step_bound(y, regime, mean, cov, M, previous).max()


# ---- 2. Fisher's identity ----------------------------------------------------------------------------------------------------------
def _dense_log_likelihood(params, regimes, observations, masks):
    """sum_{b,n} log p(y^b | s^{b,n}) by a dense Kalman filter in torch float64 (deleted rows under a mask)."""
    T = len(observations)
    B, N = regimes[0].shape
    D = params["A"].shape[-1]
    total = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        for n in range(N):
            mean, cov = params["m0"], torch.diag(params["s0"] ** 2)
            for t in range(T):
                s = int(regimes[t][b, n])
                if t > 0:
                    A = params["A"][s]
                    mean, cov = A @ mean + params["b"][s], A @ cov @ A.T + torch.diag(params["q"][s] ** 2)
                keep = np.arange(observations[t].shape[1]) if masks is None else np.flatnonzero(masks[t][b])
                if len(keep) == 0:
                    continue
                C, d, r = params["C"][s][keep], params["d"][s][keep], params["r"][s][keep]
                y = torch.from_numpy(np.asarray(observations[t][b], dtype=np.float64)[keep])
                S = C @ cov @ C.T + torch.diag(r ** 2)
                residual = y - C @ mean - d
                total = total - 0.5 * (residual @ torch.linalg.solve(S, residual) + torch.linalg.slogdet(S)[1] +
                                       len(keep) * float(np.log(2.0 * np.pi)))
                gain = cov @ C.T @ torch.linalg.inv(S)
                mean, cov = mean + gain @ residual, cov - gain @ C @ cov
                cov = 0.5 * (cov + cov.T)
    return total


def _moment_allowances(result, observations, M, D, Dy):
    """How far the statistics may lie from the exact ones, given the pass's propagated tolerances on its moments: one
    number per statistic (the largest over its entries), by the triangle inequality over every (t, b, n)."""
    tol = result["tolerances"]
    T = len(observations)
    norm = lambda m: np.sqrt((m ** 2).sum(axis=-1))
    second = [(tol["covariances"][t] + (2.0 * norm(result["means"][t]) + tol["means"][t]) * tol["means"][t]).sum()
              for t in range(T)]
    first = [np.full(result["means"][t].shape[:2], tol["means"][t]).sum() for t in range(T)]
    lagged = [(tol["cross_covariances"][t - 1] + norm(result["means"][t]) * tol["means"][t - 1] +
               norm(result["means"][t - 1]) * tol["means"][t] + tol["means"][t] * tol["means"][t - 1]).sum()
              for t in range(1, T)]
    largest_y = max(float(np.nanmax(np.abs(np.where(np.isnan(y), 0.0, y)))) for y in observations)
    return {"next_next": sum(second[1:]), "next_prev": sum(lagged) + sum(first[1:]), "prev_prev": sum(second[:-1]),
            "obs_state": largest_y * sum(first), "state_state": sum(second), "initial_state": second[0], "obs_obs": 0.0}


def _score_allowances(model, delta, N):
    """The moment allowances pushed through `score`, which is linear in the statistics: per parameter an array."""
    out = {}
    for names, cross, gram, square in ((("A", "b", "q"), "next_prev", "prev_prev", "next_next"),
                                      (("C", "d", "r"), "obs_state", "state_state", "obs_obs")):
        weights = np.concatenate([model[names[0]], model[names[1]][..., None]], axis=-1)
        reach = np.abs(weights).sum(axis=-1)
        sigma = model[names[2]]
        row = (delta[cross] + reach * delta[gram]) / sigma ** 2 / N
        out[names[0]] = np.broadcast_to(row[..., None], model[names[0]].shape)
        out[names[1]] = row
        out[names[2]] = (delta[square] + 2.0 * reach * delta[cross] + reach ** 2 * delta[gram]) / sigma ** 3 / N
    reach = 1.0 + np.abs(model["m0"])
    out["m0"] = reach * delta["initial_state"] / model["s0"] ** 2 / N
    out["s0"] = reach ** 2 * delta["initial_state"] / model["s0"] ** 3 / N
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 1), (2, 3, 2)], ids=str)
def test_fishers_identity(shape, masked):
    """`score` along given regime paths against the autograd gradient of (1/N) sum_{b,n} log p(y^b | s^{b,n}) from a dense
    Kalman filter.  Allowance: the contract pass's propagated tolerances pushed through the statistics, plus 1e-9 (1 +
    |value|) for the dense side.  Largest share of the allowance seen over the six cases: 7.0e-6."""
    (M, D, Dy), B, N, T = shape, 2, 3, 4
    model = contract.example_model(M, D, Dy)
    rng = np.random.default_rng([M, D, Dy, 47])
    regimes = [rng.integers(0, M, size=(B, N)).astype(np.int32) for _ in range(T)]
    observations = [rng.standard_normal((B, Dy)) for _ in range(T)]
    masks = None
    if masked:
        masks = _masks(T, B, Dy)
        masks[-1][:] = rng.uniform(size=(B, Dy)) < 0.6      # (the last step observed in part: it informs the smoother)
        masks[2][:] = False                                    # a step with nothing observed
        observations = _poisoned(observations, masks)
        result = missing.switching_state_pass(model, regimes, observations, masks)
    else:
        result = contract.switching_state_pass(model, regimes, observations)
    smoothed = dict(result, regimes=regimes)
    got = stats.score(stats.expected_statistics(smoothed, observations, M, masks), model)
    params = {name: torch.from_numpy(np.array(model[name])).requires_grad_(True) for name in MODEL_KEYS[2:]}
    (_dense_log_likelihood(params, regimes, observations, masks) / N).backward()
    allowance = _score_allowances(model, _moment_allowances(result, observations, M, D, Dy), N)
    worst = 0.0
    for name in MODEL_KEYS[2:]:
        want = params[name].grad.numpy()
        allowed = allowance[name] + 1e-9 * (1.0 + np.abs(want))
        error = np.abs(got[name] - want)
        worst = max(worst, float((error / allowed).max()))
        assert got[name].shape == want.shape and (error <= allowed).all(), (name, float(error.max()))
    print("largest share of the allowance", worst)


# ---- 3. stationarity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_m_step_is_a_stationary_point_of_the_score(masked):
    """The M-step maximises the function whose gradient the score is: at the new model, with the SAME statistics, the score
    of every learned entry of a visited regime is zero within the statistics' summation bound (`bounds`) pushed through the
    score — scaled by the entry's 1 / q^2 (1 / r^2, 1 / s0^2) factor."""
    B, N, M, D, Dy, T = 4, 8, 2, 3, 2, 6
    smoothed, observations = stats.example_smoothed(B, N, M, D, Dy, T)
    masks = _masks(T, B, Dy) if masked else None
    statistics = stats.expected_statistics(smoothed, observations, M, masks)
    previous = contract.example_model(M, D, Dy)
    new = stats.m_step(statistics, previous)
    got = stats.score(statistics, new)
    delta = {name: statistics["bounds"][name].max() for name in NAMES}
    allowance = _score_allowances(new, delta, N)
    for name in MODEL_KEYS[2:]:
        assert got[name].shape == np.shape(previous[name])
        assert (np.abs(got[name]) <= 2.0 * allowance[name]).all(), (name, float(np.abs(got[name]).max()), allowance[name].max())
    assert abs(new["pi0"].sum() - 1.0) < 1e-12 and (np.abs(new["Pi"].sum(axis=1) - 1.0) < 1e-12).all()


# ---- 4. exact EM with one regime ---------------------------------------------------------------------------------------------------
def test_exact_em_with_one_regime_never_lowers_the_likelihood():
    B, D, Dy, T = 3, 2, 2, 10
    truth = contract.example_model(1, D, Dy)
    rng = np.random.default_rng(48)
    z = truth["m0"] + truth["s0"] * rng.standard_normal((B, D))
    observations = []
    for t in range(T):
        if t > 0:
            z = z @ truth["A"][0].T + truth["b"][0] + truth["q"][0] * rng.standard_normal((B, D))
        observations.append(z @ truth["C"][0].T + truth["d"][0] + truth["r"][0] * rng.standard_normal((B, Dy)))
    model = {name: np.array(value) for name, value in contract.example_model(1, D, Dy, seed=5).items()}
    model["A"] = 0.5 * model["A"]
    regimes = [np.zeros((B, 1), dtype=np.int32) for _ in range(T)]
    value = lambda m: sum(contract._sequence_log_likelihood(m, [0] * T, [y[b:b + 1] for y in observations]) for b in range(B))
    values = [value(model)]
    for _ in range(5):
        result = contract.switching_state_pass(model, regimes, observations)
        statistics = stats.expected_statistics(dict(result, regimes=regimes), observations, 1)
        model = dict(model, **stats.m_step(statistics, model))
        values.append(value(model))
    for before, after in zip(values, values[1:]):
        assert after >= before - 1e-9 * (1.0 + abs(before)), values
    assert values[-1] > values[0] + 1.0, values


# ---- 5. shared parameters, regimes never visited, `learn` ----------------------------------------------------------------------------
def test_shared_unvisited_and_learn():
    B, N, M, D, Dy, T = 2, 5, 3, 2, 2, 4
    smoothed, observations = stats.example_smoothed(B, N, 2, D, Dy, T)      # regime 2 is never visited
    statistics = stats.expected_statistics(smoothed, observations, M)
    previous = contract.example_model(M, D, Dy)
    new = stats.m_step(statistics, previous)
    for name in ("A", "b", "q", "C", "d", "r"):
        assert np.array_equal(new[name][2], previous[name][2]) and not np.array_equal(new[name][:2], previous[name][:2]), name
    assert np.array_equal(new["Pi"][2], previous["Pi"][2]) and new["pi0"][2] == 0
    assert (new["Pi"][:2, 2] == 0).all() and np.abs(new["Pi"][:2].sum(axis=1) - 1.0).max() < 1e-12
    only = stats.m_step(statistics, previous, learn=("A", "b"))
    for name in MODEL_KEYS:
        assert np.array_equal(only[name], new[name] if name in ("A", "b") else previous[name]), name
    with pytest.raises(ValueError, match="learn names"):
        stats.m_step(statistics, previous, learn=("A", "Q"))
    # shared: a leading 1 stays and the estimate is the regression on the statistics summed over the regimes
    shared = dict(previous, **{name: previous[name][:1] for name in ("A", "b", "q", "r")})
    pooled = stats.m_step(statistics, shared)
    for name in ("A", "b", "q", "r"):
        assert pooled[name].shape == shared[name].shape
    for name in ("C", "d"):
        assert pooled[name].shape == previous[name].shape
    weights = statistics["next_prev"].sum(axis=0) @ np.linalg.pinv(statistics["prev_prev"].sum(axis=0), hermitian=True)
    assert np.abs(pooled["A"][0] - weights[:, :D]).max() < 1e-12 and np.abs(pooled["b"][0] - weights[:, D]).max() < 1e-12
    quad = np.diagonal(statistics["next_next"].sum(axis=0)) - 2.0 * (weights * statistics["next_prev"].sum(axis=0)).sum(axis=1) + \
        np.einsum("il,lk,ik->i", weights, statistics["prev_prev"].sum(axis=0), weights)
    assert np.abs(pooled["q"][0] - np.sqrt(quad / statistics["prev_prev"][:, D, D].sum())).max() < 1e-12
    folded, plain = stats.score(statistics, shared), stats.score(statistics, dict(shared, A=previous["A"][:1].repeat(M, axis=0)))
    assert folded["A"].shape == (1, D, D) and np.abs(folded["A"][0] - plain["A"].sum(axis=0)).max() < 1e-12
    with pytest.raises(NotImplementedError, match="both be shared"):
        stats.m_step(statistics, dict(previous, A=previous["A"][:1]))
    # a component never observed under a regime keeps its row of C, d, r
    masks = [np.ones((B, Dy), dtype=bool) for _ in range(T)]
    for mask in masks:
        mask[:, 1] = False
    unseen = stats.m_step(stats.expected_statistics(smoothed, observations, M, masks), previous)
    for name in ("C", "d", "r"):
        assert np.array_equal(unseen[name][:, 1], previous[name][:, 1]) and not np.array_equal(unseen[name][:2, 0], previous[name][:2, 0])


def test_torch_m_step_and_score_are_the_contracts():
    """`rao_blackwell.switching_m_step` and `switching_score` (plain torch: they run wherever the statistics are) against the
    NumPy contract on the same statistics."""
    from aesmc_amd import rao_blackwell
    B, N, M, D, Dy, T = 2, 6, 3, 3, 2, 5
    smoothed, observations = stats.example_smoothed(B, N, 2, D, Dy, T)
    masks = _masks(T, B, Dy)
    for mask_set in (None, masks):
        statistics = stats.expected_statistics(smoothed, observations, M, mask_set)
        as_torch = {name: torch.from_numpy(np.array(statistics[name])) for name in NAMES}
        as_torch.update(batch_size=B, num_trajectories=N, num_timesteps=T)
        for shared in ((), ("q", "r"), ("A", "b", "q", "C", "d", "r")):
            previous = contract.example_model(M, D, Dy)
            previous = dict(previous, **{name: previous[name][:1] for name in shared})
            module = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(np.array(previous[name])) for name in MODEL_KEYS])
            for learn in (MODEL_KEYS, ("A", "q"), ("d", "r", "s0", "Pi")):
                want = stats.m_step(statistics, previous, learn)
                got = rao_blackwell.switching_m_step(as_torch, module, learn)
                assert isinstance(got, rao_blackwell.SwitchingLinearGaussian)
                for name in MODEL_KEYS:
                    value = getattr(got, name).numpy()
                    assert value.shape == np.shape(want[name]), name
                    assert np.abs(value - want[name]).max() <= 1e-10 * (1.0 + np.abs(want[name]).max()), (name, shared, learn)
            want, got = stats.score(statistics, previous), rao_blackwell.switching_score(as_torch, module)
            for name in MODEL_KEYS:
                assert tuple(got[name].shape) == np.shape(want[name]), name
                assert np.abs(got[name].numpy() - want[name]).max() <= 1e-10 * (1.0 + np.abs(want[name]).max()), (name, shared)
    with pytest.raises(ValueError, match="learn names"):
        rao_blackwell.switching_m_step(as_torch, module, ("A", "Q"))
    with pytest.raises(ValueError, match="what switching_expected_statistics returns"):
        rao_blackwell.switching_m_step({"next_prev": as_torch["next_prev"]}, module)
    with pytest.raises(ValueError, match="must be a SwitchingLinearGaussian"):
        rao_blackwell.switching_score(as_torch, previous)
    other = contract.example_model(M, D + 1, Dy)
    with pytest.raises(ValueError, match="the model has"):
        rao_blackwell.switching_score(as_torch, rao_blackwell.SwitchingLinearGaussian(
            *[torch.from_numpy(np.array(other[name])) for name in MODEL_KEYS]))


# ---- 6. the host logic on a provider double ------------------------------------------------------------------------------------------
class StatisticsDouble(OracleKernels):
    """The suite's oracle provider plus K45 / K46 and their finish from the NumPy contract; every call is recorded."""

    def __init__(self):
        super().__init__()
        self.calls, self.blocks = [], {}

    def read_flags(self, device):
        self.calls.append("read_flags")
        return super().read_flags(device)

    def switching_statistics_columns(self, latent_dim, observation_dim, masked):
        return stats.layout(latent_dim, observation_dim, masked)["columns"]

    def switching_statistics_step(self, observation, regime, mean, cov, num_regimes, previous=None, observed=None, block=0,
                                  accumulate=False):
        self.calls.append(("step", previous is not None, observed is not None, block, bool(accumulate)))
        step, _, flags = stats.statistics_step(
            observation.numpy(), regime.numpy(), mean.numpy(), cov.numpy(), num_regimes,
            None if previous is None else tuple(part.numpy() for part in previous), None if observed is None else observed.numpy())
        self._flags |= flags
        self.blocks[block] = self.blocks[block] + step if accumulate else step

    def switching_statistics_finish(self, like, batch_size, num_trajectories, latent_dim, observation_dim, masked, block=0):
        self.calls.append(("finish", block))
        return torch.from_numpy(self.blocks[block].copy())


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = StatisticsDouble()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _torch_pass(B, N, M, D, Dy, T):
    smoothed, observations = stats.example_smoothed(B, N, M, D, Dy, T)
    return ({key: [torch.from_numpy(value) for value in values] for key, values in smoothed.items()},
            [torch.from_numpy(y) for y in observations], smoothed, observations)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_host_pass_on_the_double(backend, masked):
    from aesmc_amd import rao_blackwell
    B, N, M, D, Dy, T = 2, 4, 3, 2, 2, 4
    smoothed, observations, host, host_observations = _torch_pass(B, N, M, D, Dy, T)
    masks = _masks(T, B, Dy)
    masks[1] = None
    observed = [None if mask is None else torch.from_numpy(mask) for mask in masks] if masked else None
    got = rao_blackwell.switching_expected_statistics(smoothed, observations, M, observed=observed)
    want = stats.expected_statistics(host, host_observations, M, masks if masked else None)
    for name in NAMES:
        assert np.abs(got[name].numpy() - want[name]).max() <= 2.0 * want["bounds"][name].max(), name
    assert (got["batch_size"], got["num_trajectories"], got["num_timesteps"]) == (B, N, T)
    # one launch per timestep, t = 0 into its own block, nothing but the steps between the first and the last launch, then
    # the two finishes and ONE read
    steps = [("step", False, masked, 0, False), ("step", True, masked, 1, False)] + [("step", True, masked, 1, True)] * (T - 2)
    assert backend.calls == steps + [("finish", 0), ("finish", 1), "read_flags"]
    if not masked:
        assert got["state_state"].stride(1) == 0
    # T == 1: only the t = 0 form, one finish
    backend.calls.clear()
    one = rao_blackwell.switching_expected_statistics({key: values[:1] if key != "cross_covariances" else [] for key, values in
                                                       smoothed.items()}, observations[:1], M)
    assert backend.calls == [("step", False, False, 0, False), ("finish", 0), "read_flags"]
    assert float(one["transition_counts"].abs().sum()) == 0 and float(one["initial_counts"].sum()) == B * N
    # the model in place of M
    model = contract.example_model(M, D, Dy)
    module = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(np.array(model[name])) for name in MODEL_KEYS])
    again = rao_blackwell.switching_expected_statistics(smoothed, observations, module, observed=observed)
    assert all(torch.equal(again[name], got[name]) for name in NAMES)


def test_host_refusals_on_the_double(backend):
    from aesmc_amd import rao_blackwell
    run = rao_blackwell.switching_expected_statistics
    B, N, M, D, Dy, T = 2, 4, 3, 2, 2, 3
    smoothed, observations, _, _ = _torch_pass(B, N, M, D, Dy, T)
    with pytest.raises(ValueError, match="at least one timestep"):
        run(smoothed, [], M)
    with pytest.raises(ValueError, match="at least 1"):
        run(smoothed, observations, 0)
    with pytest.raises(ValueError, match="must be a dict with"):
        run({key: value for key, value in smoothed.items() if key != "regimes"}, observations, M)
    with pytest.raises(ValueError, match="must hold 2 tensors"):
        run(dict(smoothed, cross_covariances=smoothed["cross_covariances"][:1]), observations, M)
    with pytest.raises(ValueError, match=r"smoothed\['regimes'\]\[1\] must be"):
        run(dict(smoothed, regimes=[r.to(torch.int64) if t == 1 else r for t, r in enumerate(smoothed["regimes"])]),
            observations, M)
    with pytest.raises(ValueError, match=r"smoothed\['cross_covariances'\]\[0\] must be"):
        run(dict(smoothed, cross_covariances=[x[:, :, :1] for x in smoothed["cross_covariances"]]), observations, M)
    with pytest.raises(ValueError, match="observations must be"):
        run(smoothed, [observations[0], observations[1][:, :1], observations[2]], M)
    with pytest.raises(ValueError, match="batch rows"):
        run(smoothed, [y[:1] for y in observations], M)
    with pytest.raises(ValueError, match="observed must be None or hold one entry per timestep"):
        run(smoothed, observations, M, observed=[None])
    model = contract.example_model(M, D + 1, Dy)
    module = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(np.array(model[name])) for name in MODEL_KEYS])
    with pytest.raises(ValueError, match="the model has D = 3"):
        run(smoothed, observations, module)
    with pytest.raises(NotImplementedError, match="17 regimes"):
        run(smoothed, observations, 17)
    wide, wide_observations, _, _ = _torch_pass(1, 1, 1, 9, 1, 2)
    with pytest.raises(NotImplementedError, match="latent of 9"):
        run(wide, wide_observations, 1)
    tall, tall_observations, _, _ = _torch_pass(1, 1, 1, 1, 9, 2)
    with pytest.raises(NotImplementedError, match="observation of 9"):
        run(tall, tall_observations, 1)
    assert backend.calls == []
    # N == 0: zeros without a launch
    empty, empty_observations, _, _ = _torch_pass(B, 0, M, D, Dy, T)
    zeros = run(empty, empty_observations, M)
    assert backend.calls == [] and zeros["num_trajectories"] == 0
    assert tuple(zeros["next_prev"].shape) == (M, D, D + 1) and tuple(zeros["state_state"].shape) == (M, Dy, D + 1, D + 1)
    assert all(float(zeros[name].abs().sum()) == 0 for name in NAMES)
    # a regime outside [0, M): ValueError at the end, after the one read, the flag gone
    bad = dict(smoothed, regimes=[r.clone() for r in smoothed["regimes"]])
    bad["regimes"][1][0, 2] = M
    with pytest.raises(ValueError, match=r"outside \[0, M\)"):
        run(bad, observations, M)
    assert backend.calls.count("read_flags") == 1 and backend.read_flags(None) == 0
    # a NaN moment is an error
    nan = dict(smoothed, means=[m.clone() for m in smoothed["means"]])
    nan["means"][2][1, 1, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="nan"):
        run(nan, observations, M)


# ---- 7. the status codes of the three C entries --------------------------------------------------------------------------------------
STEP = ("y_dtype", "y", "regime", "regime_prev", "mean_prev", "cov_prev", "cross", "mean", "cov", "workspace", "accumulate", "flags",
        "B", "N", "M", "D", "Dy", "stream")
MASKED_STEP = STEP[:2] + ("observed",) + STEP[2:]
FINISH = ("workspace", "out", "masked", "B", "N", "D", "Dy", "stream")
STORED = ("regime_prev", "mean_prev", "cov_prev", "cross")
LIMIT = 0x7fffffff


class Entry:
    """One C entry with a valid set of made-up arguments (every pointer a distinct multiple of 64, B = 0), the conventions of
    tests/test_switching_abi_status.py: no case here can launch a kernel."""

    def __init__(self, name, order):
        self.name, self.order = name, order
        self.valid = {arg: 64 * (i + 1) for i, arg in enumerate(order)}
        self.valid.update({arg: None for arg in STORED if arg in order})
        self.valid.update(y_dtype=_lib.F64, accumulate=0, masked=0, B=0, N=3, M=2, D=2, Dy=1, stream=None)

    def __call__(self, **changes):
        args = dict(self.valid, **changes)
        return getattr(_lib.load(), "aesmc_switching_" + self.name)(*[args[arg] for arg in self.order])

    def later(self, **changes):
        return self(**dict({arg: 4096 + 64 * i for i, arg in enumerate(STORED)}, **changes))


STEPS = [Entry("moment_statistics", STEP), Entry("masked_moment_statistics", MASKED_STEP)]
FINISHER = Entry("statistics_finish", FINISH)
ids = dict(ids=lambda entry: entry.name)


def test_statistics_getters():
    lib = _lib.load()
    for D, Dy, masked in ((1, 1, 0), (2, 1, 1), (5, 3, 0), (8, 8, 1)):
        assert lib.aesmc_switching_statistics_columns(D, Dy, masked) == stats.layout(D, Dy, bool(masked))["columns"]
        assert lib.aesmc_switching_statistics_workspace_bytes(D, Dy, masked) > 0
    assert lib.aesmc_switching_statistics_workspace_bytes(8, 8, 0) == 512 * 19 * 256 * 8      # 8 + 11 tiles of 16 columns
    assert lib.aesmc_switching_statistics_workspace_bytes(5, 3, 1) == lib.aesmc_switching_statistics_workspace_bytes(8, 4, 1)
    for D, Dy in ((0, 1), (1, 0), (9, 1), (1, 9)):
        assert lib.aesmc_switching_statistics_columns(D, Dy, 0) == 0 and lib.aesmc_switching_statistics_workspace_bytes(D, Dy, 0) == 0


@pytest.mark.parametrize("entry", STEPS, **ids)
def test_statistics_step_status(entry):
    masked = "observed" in entry.order
    assert entry() == 0 and entry(B=2, N=0) == 0 and entry.later() == 0 and entry.later(B=2, N=0) == 0
    assert entry(B=-1) == 1 and entry(N=-1) == 1
    for arg in ("y", "regime", "mean", "cov", "workspace"):
        assert entry(**{arg: None}) == 1 and entry.later(**{arg: None}) == 1, arg
    assert entry(flags=None) == 0
    for extent in ("M", "D", "Dy"):
        assert entry(**{extent: 0}) == 1, extent
    for tag in (-1, 2, 5):
        assert entry(y_dtype=tag) == 1
    assert entry(y=entry.valid["y"] + 4) == 1 and entry(y=entry.valid["y"] + 4, y_dtype=_lib.F32) == 0
    assert entry(y=entry.valid["y"] + 2, y_dtype=_lib.F32) == 1
    assert entry(accumulate=1) == 0 and entry(accumulate=2) == 1 and entry(accumulate=-1) == 1
    # the operands of time t-1 come together
    for given in range(1, 15):
        some = {arg: 4096 + 64 * i for i, arg in enumerate(STORED) if given >> i & 1}
        assert entry(**some) == 1, sorted(some)
    # misalignment
    later = {arg: 4096 + 64 * i for i, arg in enumerate(STORED)}
    for arg in ("regime", "regime_prev", "mean_prev", "cov_prev", "cross", "mean", "cov", "workspace", "flags"):
        base = dict(entry.valid, **later)
        assert entry(**dict(later, **{arg: base[arg] + (2 if arg in ("regime", "regime_prev", "flags") else 4)})) == 1, arg
    # the output is none of the inputs
    for arg in ("y", "regime", "mean", "cov", "flags") + (("observed",) if masked else ()):
        assert entry(workspace=entry.valid[arg]) == 1, arg
    for arg in STORED:
        assert entry.later(workspace=later[arg]) == 1, arg
    if masked:
        assert entry(observed=None) == 1 and entry(observed=entry.valid["observed"] + 1) == 0      # bytes: no alignment
    # the orderings: invalid beside unsupported is invalid; an unsupported extent of an empty launch is not looked at
    for extent in ({"D": 9}, {"Dy": 9}, {"M": 17}):
        assert entry(**extent) == 0 and entry(B=2, N=0, **extent) == 0
        assert entry(mean=None, **extent) == 1 and entry(accumulate=3, **extent) == 1


def test_statistics_finish_status():
    entry = FINISHER
    assert entry() == 0 and entry(B=2, N=0) == 0 and entry(masked=1) == 0
    assert entry(B=-1) == 1 and entry(N=-1) == 1 and entry(D=0) == 1 and entry(Dy=0) == 1 and entry(masked=2) == 1
    assert entry(workspace=None) == 1 and entry(out=None) == 1 and entry(out=entry.valid["workspace"]) == 1
    assert entry(workspace=entry.valid["workspace"] + 4) == 1 and entry(out=entry.valid["out"] + 4) == 1
    for extent in ({"D": 9}, {"Dy": 9}):
        assert entry(**extent) == 0 and entry(out=None, **extent) == 1


@no_gpu
@pytest.mark.parametrize("entry", STEPS + [FINISHER], **ids)
def test_statistics_unsupported(entry):
    calls = (entry,) if entry is FINISHER else (entry, entry.later)
    for call in calls:
        assert call(D=9, B=2) == 2 and call(Dy=9, B=2) == 2
        if entry is not FINISHER:
            assert call(M=17, B=2) == 2
        assert call(B=LIMIT + 1, N=1) == 2 and call(B=1, N=LIMIT + 1) == 2
        assert call(B=1, N=LIMIT // 64 + 1) == 2 and call(B=1 << 16, N=1 << 16) == 2
    assert entry(B=1, N=LIMIT // 64) == 3        # the bound itself passes every check; without a device the launch fails
