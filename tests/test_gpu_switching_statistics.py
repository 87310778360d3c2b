"""The switching-model EM statistics on the device: K45 / K46 (aesmc_switching_moment_statistics,
aesmc_switching_masked_moment_statistics) with aesmc_switching_statistics_finish against their NumPy contract
(aesmc_amd/testing/switching_statistics.py) within TWICE the contract's summation bound (kernel and contract each sum in
their own order; nothing looser), the kernels' conventions, and `switching_expected_statistics` / `switching_m_step` end to
end."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_missing as missing
from aesmc_amd.testing import switching_statistics as stats

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
# (B, N, M, D, Dy): one lane; a wavefront's edge; a workgroup's edge with every column tile of the largest extents; several
# workgroups with padded extents; all 16 rows; five workgroups
SHAPES = [(1, 1, 1, 1, 1), (3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3), (1, 257, 16, 8, 1), (2, 1025, 2, 3, 2)]


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device="cuda"):
    return None if array is None else torch.from_numpy(np.ascontiguousarray(array)).to(device)


def _case(B, N, M, D, Dy, dtype, masked, seed=0):
    y, regime, mean, cov, previous = stats.example_step(B, N, M, D, Dy, observation_dtype=dtype, seed=seed)
    mask = missing.example_mask(B, Dy, variant=seed % 3) if masked else None
    return y, regime, mean, cov, previous, mask


def _launch(provider, case, M, later, block=0, accumulate=False, y=None):
    observation, regime, mean, cov, previous, mask = case
    provider.switching_statistics_step(
        _dev(observation if y is None else y), _dev(regime), _dev(mean), _dev(cov), M,
        previous=tuple(_dev(part) for part in previous) if later else None, observed=_dev(mask), block=block,
        accumulate=accumulate)


def _finish(provider, case, block=0):
    mean, observation, mask = case[2], case[0], case[5]
    B, N, D = mean.shape
    return provider.switching_statistics_finish(_dev(mean), B, N, D, observation.shape[1], mask is not None, block=block)


def _expected(case, M, later):
    y, regime, mean, cov, previous, mask = case
    return stats.statistics_step(y, regime, mean, cov, M, previous if later else None, mask)


def _within(what, got, want, magnitude, terms):
    bound = 2.0 * (terms + 4) * stats.UNIT * magnitude
    error = np.abs(got - want)
    share = float((error / np.where(bound > 0, bound, 1.0)).max())
    print(what, "largest error", error.max(), "largest share of the allowance", share)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert (error <= bound).all(), (what, float(error.max()), share)


@pytest.mark.parametrize("masked", [False, True], ids=["k45", "k46"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["y32", "y64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_contract(shape, dtype, masked):
    B, N, M, D, Dy = shape
    provider = _provider()
    case, second = _case(B, N, M, D, Dy, dtype, masked), _case(B, N, M, D, Dy, dtype, masked, seed=1)
    assert int(provider._lib.aesmc_switching_statistics_columns(D, Dy, int(masked))) == stats.layout(D, Dy, masked)["columns"]
    for later in (False, True):
        _launch(provider, case, M, later)
        want, magnitude, flags = _expected(case, M, later)
        assert flags == 0
        _within(("one launch", later), _finish(provider, case).cpu().numpy(), want, magnitude, B * N)
    # two launches accumulated: a later step, then another one
    _launch(provider, case, M, True, block=1)
    _launch(provider, second, M, True, block=1, accumulate=True)
    first, first_magnitude, _ = _expected(case, M, True)
    other, other_magnitude, _ = _expected(second, M, True)
    _within("accumulated", _finish(provider, case, block=1).cpu().numpy(), first + other, first_magnitude + other_magnitude,
            2 * B * N)
    # the t = 0 form accumulated on a later step leaves the transition block as it was
    _launch(provider, second, M, False, block=1, accumulate=True)
    third, third_magnitude, _ = _expected(second, M, False)
    _within("three", _finish(provider, case, block=1).cpu().numpy(), first + other + third,
            first_magnitude + other_magnitude + third_magnitude, 3 * B * N)
    assert provider.read_flags(torch.device("cuda")) == 0


@pytest.mark.parametrize("masked", [False, True], ids=["k45", "k46"])
def test_out_of_range_regimes_contribute_nothing(masked):
    B, N, M, D, Dy = 2, 300, 4, 5, 3
    provider = _provider()
    case = _case(B, N, M, D, Dy, np.float64, masked)
    clean, magnitude, _ = _expected(case, M, True)
    y, regime, mean, cov, previous, mask = case
    regime, regime_prev = regime.copy(), previous[0].copy()
    regime[0, 3], regime[1, 17], regime[1, 299] = M, -1, 1 << 20
    regime_prev[0, 9], regime_prev[0, 258], regime_prev[1, 5] = M, -1, 1 << 20
    bad = (y, regime, mean, cov, (regime_prev,) + previous[1:], mask)
    want, magnitude, flags = _expected(bad, M, True)
    assert flags == stats.FLAG_INDEX_OUT_OF_RANGE and not np.array_equal(want, clean)
    _launch(provider, bad, M, True)
    got = _finish(provider, bad).cpu().numpy()
    assert provider.read_flags(torch.device("cuda")) == stats.FLAG_INDEX_OUT_OF_RANGE
    _within("without the six", got, want, magnitude, B * N)
    # the t = 0 form looks at the current regime alone
    _launch(provider, bad, M, False)
    got = _finish(provider, bad).cpu().numpy()
    assert provider.read_flags(torch.device("cuda")) == stats.FLAG_INDEX_OUT_OF_RANGE
    want, magnitude, _ = _expected(bad, M, False)
    _within("t = 0", got, want, magnitude, B * N)


def test_unobserved_values_are_never_used():
    B, N, M, D, Dy = 3, 70, 3, 4, 3
    provider = _provider()
    case = _case(B, N, M, D, Dy, np.float64, True)
    mask = case[5]
    assert (~mask).any() and mask.any()
    poisoned = case[0].copy()
    poisoned[~mask] = np.where(np.arange((~mask).sum()) % 2 == 0, np.nan, np.inf)
    _launch(provider, case, M, True)
    plain = _finish(provider, case)
    _launch(provider, case, M, True, y=poisoned)
    got = _finish(provider, case)
    assert torch.isfinite(got).all() and torch.equal(got, plain)
    assert provider.read_flags(torch.device("cuda")) == 0


@pytest.mark.parametrize("masked", [False, True], ids=["k45", "k46"])
def test_same_operands_same_bits_and_overwrite_reads_nothing(masked):
    B, N, M, D, Dy = 2, 1025, 2, 3, 2
    provider = _provider()
    case = _case(B, N, M, D, Dy, np.float64, masked)
    _launch(provider, case, M, True)
    first = _finish(provider, case)
    held, _ = provider._switching_statistics_workspace(torch.device("cuda", torch.cuda.current_device()), D, Dy, masked, 0)
    held.view(torch.float64).fill_(float("nan"))      # accumulate = 0 must not read what the workspace holds
    _launch(provider, case, M, True)
    again = _finish(provider, case)
    assert torch.isfinite(again).all() and torch.equal(first, again)
    held.view(torch.float64).fill_(float("nan"))
    _launch(provider, case, M, False)                  # the t = 0 form writes zeros over the transition block
    initial = _finish(provider, case)
    where = stats.layout(D, Dy, masked)
    assert torch.isfinite(initial).all() and bool((initial[:, where["counts"].start:] == 0).all())


def _torch_model(ops, device="cuda"):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(np.array(ops[name])) for name in MODEL_KEYS]).to(device)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_expected_statistics_end_to_end(masked):
    """switching_state_smooth(return_trajectories=True) -> switching_expected_statistics on the device against the contract's
    `expected_statistics` on the same moments copied to the host, within twice its bound, at T = 4."""
    from aesmc_amd import rao_blackwell
    B, N, M, D, Dy, T = 2, 70, 3, 3, 2, 4
    ops = contract.example_model(M, D, Dy)
    model = _torch_model(ops)
    rng = np.random.default_rng(7)
    observations = [_dev(rng.standard_normal((B, Dy))) for _ in range(T)]
    regimes = [_dev(rng.integers(0, M, size=(B, N)).astype(np.int32)) for _ in range(T)]
    observed = None
    if masked:
        observed = [None] + [_dev(mask) for mask in missing.example_masks(T, B, Dy)[1:]]
    smoothed = rao_blackwell.switching_state_smooth(observations, model, regimes, return_trajectories=True, observed=observed)
    smoothed["regimes"] = regimes
    got = rao_blackwell.switching_expected_statistics(smoothed, observations, model, observed=observed)
    host = {key: [tensor.cpu().numpy() for tensor in smoothed[key]]
            for key in ("regimes", "means", "covariances", "cross_covariances")}
    want = stats.expected_statistics(host, [y.cpu().numpy() for y in observations], M,
                                     None if observed is None else [None if m is None else m.cpu().numpy() for m in observed])
    assert (got["batch_size"], got["num_trajectories"], got["num_timesteps"]) == (B, N, T)
    for name, bound in want["bounds"].items():
        value = got[name].cpu().numpy()
        error = np.abs(value - want[name])
        print(name, "largest error", error.max(), "largest bound", 2.0 * bound.max())
        assert value.shape == want[name].shape and (error <= 2.0 * bound).all(), name
    assert float(got["initial_counts"].sum()) == B * N and float(got["transition_counts"].sum()) == (T - 1) * B * N
    if not masked:
        assert got["state_state"].stride(1) == 0


def test_device_em_does_not_lower_the_likelihood():
    """M = 1: nothing is sampled and EM is exact — `kalman_log_likelihood` summed over the batch does not fall over three
    iterations by more than 1e-9 (1 + |value|), and rises from a perturbed start."""
    from aesmc_amd import rao_blackwell
    B, D, Dy, T = 4, 2, 2, 12
    truth = _torch_model(contract.example_model(1, D, Dy))
    observations = truth.simulate(T, B, seed=3)
    start = contract.example_model(1, D, Dy, seed=5)
    start["A"] = 0.5 * start["A"]
    model = _torch_model(start)
    regimes = [torch.zeros((B, 1), dtype=torch.int32, device="cuda") for _ in range(T)]
    values = [float(rao_blackwell.kalman_log_likelihood(observations, model)[0].sum())]
    for _ in range(3):
        smoothed = rao_blackwell.switching_state_smooth(observations, model, regimes, return_trajectories=True)
        smoothed["regimes"] = regimes
        statistics = rao_blackwell.switching_expected_statistics(smoothed, observations, model)
        model = rao_blackwell.switching_m_step(statistics, model)
        values.append(float(rao_blackwell.kalman_log_likelihood(observations, model)[0].sum()))
    print("log-likelihoods", values)
    for before, after in zip(values, values[1:]):
        assert after >= before - 1e-9 * (1.0 + abs(before))
    assert values[-1] > values[0]


def test_refusals_leave_the_outputs_as_they_were():
    from aesmc_amd import _lib
    provider = _provider()
    lib = _lib.load()
    B, N, M, D, Dy = 2, 7, 2, 2, 1
    y, regime, mean, cov, previous, _ = _case(B, N, M, D, Dy, np.float64, False)
    y, regime, mean, cov = _dev(y), _dev(regime), _dev(mean), _dev(cov)
    columns = stats.layout(D, Dy, False)["columns"]
    workspace = torch.full((int(lib.aesmc_switching_statistics_workspace_bytes(D, Dy, 0)) // 8,), 7.0, dtype=torch.float64,
                           device="cuda")
    out = torch.full((16, columns), 5.0, dtype=torch.float64, device="cuda")
    flags = provider.flags(torch.device("cuda"))
    step = lambda **change: lib.aesmc_switching_moment_statistics(*[dict(dict(
        y_dtype=_lib.F64, y=y.data_ptr(), regime=regime.data_ptr(), regime_prev=None, mean_prev=None, cov_prev=None, cross=None,
        mean=mean.data_ptr(), cov=cov.data_ptr(), workspace=workspace.data_ptr(), accumulate=0, flags=flags.data_ptr(), B=B, N=N,
        M=M, D=D, Dy=Dy, stream=None), **change)[key] for key in (
            "y_dtype", "y", "regime", "regime_prev", "mean_prev", "cov_prev", "cross", "mean", "cov", "workspace", "accumulate",
            "flags", "B", "N", "M", "D", "Dy", "stream")])
    finish = lambda **change: lib.aesmc_switching_statistics_finish(*[dict(dict(
        workspace=workspace.data_ptr(), out=out.data_ptr(), masked=0, B=B, N=N, D=D, Dy=Dy, stream=None), **change)[key]
        for key in ("workspace", "out", "masked", "B", "N", "D", "Dy", "stream")])
    assert step(accumulate=2) == 1 and step(regime_prev=regime.data_ptr()) == 1 and step(workspace=mean.data_ptr()) == 1
    assert step(M=17) == 2 and step(D=9) == 2 and step(y_dtype=3) == 1 and step(B=0) == 0
    assert finish(out=workspace.data_ptr()) == 1 and finish(masked=2) == 1 and finish(D=9) == 2 and finish(N=0) == 0
    torch.cuda.synchronize()
    assert bool((workspace == 7.0).all()) and bool((out == 5.0).all())
    assert step() == 0 and finish() == 0
    torch.cuda.synchronize()
    want, magnitude, _ = stats.statistics_step(y.cpu().numpy(), regime.cpu().numpy(), mean.cpu().numpy(), cov.cpu().numpy(), M)
    _within("after the refusals", out.cpu().numpy(), want, magnitude, B * N)
    assert provider.read_flags(torch.device("cuda")) == 0
