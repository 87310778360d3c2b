"""The simulation smoother of switching linear-Gaussian models on the device: kernel K47 (aesmc_switching_state_draw) against its
NumPy contract (aesmc_amd/testing/switching_state_draw.py) within the contract's bound — step by step and as a pass —, the
exactness test against the independent two-filter kernels K34 / K36, the degenerate models, the conventions, and
`aesmc_amd.rao_blackwell.switching_sample_states` end to end.

Pivots near a threshold: every case asserts from the contract alone that each pivot of both factorisations lies further from
its threshold than 4 times its running bound (`clearance` > 1), so that both sides keep and drop the same columns."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_state_draw as draw
from tests.test_switching_state_draw_contract import SHAPES, affine_moments, check_degenerate, degenerate_case, exactness_case

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
# The largest deviation of K47's float64 contract from K36's (`switching_state_pass`, under a mask `switching_missing`'s) over
# SHAPES in `exactness_case`, plain and masked, measured on the CPU: means 1.0e-15, covariances 3.4e-16, lag-one
# cross-covariances 1.5e-15 (all at (16, 8, 8)).  Times 8: the margin for the device's fused multiply-adds and reassociation
# on both sides.
MEASURED = {"means": 1.0e-15, "covariances": 3.4e-16, "cross_covariances": 1.5e-15}


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


def _device_draw(provider, device, model, regimes, means, covs, noise, following=None):
    """K47 on host arrays: T-lists are stacked; returns states [T,B,N,D] as an array."""
    ops = {name: _dev(value, device) for name, value in model.items()}
    stack = lambda parts: _dev(np.stack(parts), device)
    out = provider.switching_state_draw(ops, stack(regimes), stack(means), stack(covs), stack(noise),
                                        None if following is None else tuple(_dev(part, device) for part in following))
    return out.cpu().numpy()


def _case(M, D, Dy, B, N, T, seed=0):
    rng = np.random.default_rng([seed, M, D, Dy, B, N, T])
    model = contract.example_model(M, D, Dy, seed=1)
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    observations = [rng.standard_normal((B, Dy)) for _ in range(T)]
    noise = [rng.standard_normal((B, N, D)) for _ in range(T)]
    return model, regimes, observations, noise


@pytest.mark.parametrize("N", [1, 65, 257])      # a lane alone, a tail past a wavefront, a tail past a workgroup
@pytest.mark.parametrize("M,D,Dy", SHAPES)
def test_the_kernel_equals_the_contract_within_its_bound(hip_device, M, D, Dy, N):
    """As a pass (T = 1, 2, 5: one launch on the contract's filtered moments, against the tolerance the contract accumulates)
    and step-wise (T = 1 with `following`, every step of the longest pass fed the contract's z_{t+1}): within 2 x the bound."""
    provider = _provider()
    B = 2
    for T in (1, 2, 5):
        model, regimes, observations, noise = _case(M, D, Dy, B, N, T)
        want = draw.state_draw_pass(model, regimes, observations, noise)
        assert want["flags"] == 0 and want["clearance"] > 1
        got = _device_draw(provider, hip_device, model, regimes, want["filtered_means"], want["filtered_covariances"], noise)
        assert provider.read_flags(hip_device) == 0
        assert got.shape == (T, B, N, D) and got.dtype == np.float64
        for t in range(T):
            error, allowed = np.abs(got[t] - want["states"][t]), 2 * want["tolerances"]["states"][t]
            print("T", T, "t", t, "largest error", error.max(), "of allowance", (error / allowed).max())
            assert (error <= allowed).all(), (T, t)
    for t in range(T - 1):
        following = (regimes[t + 1], want["states"][t + 1])
        args = (model, following[0], want["filtered_means"][t], want["filtered_covariances"][t], following[1], noise[t])
        bound, clearance = draw.state_draw_step_bound(*args)
        got = _device_draw(provider, hip_device, model, regimes[t:t + 1], [args[2]], [args[3]], [noise[t]], following)[0]
        error = np.abs(got - want["states"][t])
        print("step", t, "largest error", error.max(), "of 2 x bound", (error / (2 * bound)).max())
        assert clearance > 1 and (error <= 2 * bound).all(), t
    assert provider.read_flags(hip_device) == 0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,D,Dy", SHAPES)
def test_the_pass_spans_the_two_filter_smoother_on_the_device(hip_device, M, D, Dy, masked):
    """The exactness test of the CPU suite on the device: `switching_sample_states` on zero and unit noise gives mu and W of
    z = mu + W eps; mu, the diagonal and the lag-one blocks of W W^T against `switching_state_smooth(...,
    return_trajectories=True)` — K34 and K36, which share nothing with K47 but the forward filter."""
    from aesmc_amd import rao_blackwell
    model, regimes, observations, observed, noise = exactness_case(M, D, Dy, masked)
    assert draw.state_draw_pass(model, regimes, observations, noise, observed)["clearance"] > 1
    slg = _torch_model(model, hip_device)
    ys = [_dev(y, hip_device) for y in observations]
    masks = None if observed is None else [_dev(mask, hip_device) for mask in observed]
    paths = [_dev(regime, hip_device) for regime in regimes]
    out = rao_blackwell.switching_sample_states(ys, slg, paths, noise=[_dev(eps, hip_device) for eps in noise], observed=masks)
    smooth = rao_blackwell.switching_state_smooth(ys, slg, [path[:, :1] for path in paths], return_trajectories=True,
                                                  observed=masks)
    got = dict(zip(("means", "covariances", "cross_covariances"), affine_moments([z.cpu().numpy() for z in out["states"]], D)))
    want = {"means": np.stack([m[0, 0].cpu().numpy() for m in smooth["means"]]),
            "covariances": np.stack([contract.unpack(c[0, 0].cpu().numpy(), D) for c in smooth["covariances"]]),
            "cross_covariances": np.stack([x[0, 0].cpu().numpy() for x in smooth["cross_covariances"]])}
    assert torch.equal(out["log_likelihood"][:, :1], smooth["log_likelihood"])
    for key in got:
        error = float(np.abs(got[key] - want[key]).max())
        print(key, "deviation from K36", error, "allowed", 8 * MEASURED[key])
        assert error <= 8 * MEASURED[key], key


@pytest.mark.parametrize("variant", ["q1", "q", "s0", "both"])
def test_degenerate_models_on_the_device(hip_device, variant):
    """q = 0 components, P = 0 and both: no NaN, no flag, the same properties as the contract's draws and within 2 x its
    accumulated tolerance of them."""
    provider = _provider()
    model, regimes, observations, noise = degenerate_case(variant)
    want = draw.state_draw_pass(model, regimes, observations, noise)
    assert want["flags"] == 0 and want["clearance"] > 1
    got = _device_draw(provider, hip_device, model, regimes, want["filtered_means"], want["filtered_covariances"], noise)
    assert provider.read_flags(hip_device) == 0
    check_degenerate(variant, model, regimes, list(got), want["filtered_means"], want["tolerances"]["states"])
    for t in range(len(regimes)):
        assert (np.abs(got[t] - want["states"][t]) <= 2 * want["tolerances"]["states"][t]).all(), t


def test_regimes_out_of_range_chunks_and_the_same_bits(hip_device):
    provider = _provider()
    M, D, Dy, B, N, T = 3, 3, 2, 2, 300, 5
    model, regimes, observations, noise = _case(M, D, Dy, B, N, T, seed=1)
    filtered = draw.state_draw_pass(model, regimes, observations, noise)
    means, covs = filtered["filtered_means"], filtered["filtered_covariances"]
    clean = _device_draw(provider, hip_device, model, regimes, means, covs, noise)
    assert provider.read_flags(hip_device) == 0 and np.isfinite(clean).all()
    # the same inputs, the same bits
    assert np.array_equal(clean, _device_draw(provider, hip_device, model, regimes, means, covs, noise))
    # a pass in chunks: steps 0 .. 2 with the regime and the drawn state of step 3 handed over, bit for bit
    chunk = _device_draw(provider, hip_device, model, regimes[:3], means[:3], covs[:3], noise[:3], (regimes[3], clean[3]))
    assert np.array_equal(chunk, clean[:3])
    # a regime outside [0, M) at step t: NaN at steps <= t-1 of that trajectory only, and the flag; regimes[0] is not read
    bad = [regime.copy() for regime in regimes]
    bad[3][1, 299], bad[1][0, 3], bad[4][1, 256], bad[0][0, 7] = M, -1, 1 << 20, M
    got = _device_draw(provider, hip_device, model, bad, means, covs, noise)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    gone = np.zeros((T, B, N), dtype=bool)
    gone[:3, 1, 299] = gone[:1, 0, 3] = gone[:4, 1, 256] = True
    assert np.isnan(got[gone]).all() and np.array_equal(got[~gone], clean[~gone])
    # ... and in `following`: the whole trajectory
    regime_next = regimes[3].copy()
    regime_next[0, 258] = M
    got = _device_draw(provider, hip_device, model, regimes[:3], means[:3], covs[:3], noise[:3], (regime_next, clean[3]))
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    gone = np.zeros((3, B, N), dtype=bool)
    gone[:, 0, 258] = True
    assert np.isnan(got[gone]).all() and np.array_equal(got[~gone], clean[:3][~gone])
    # wrapper validation and the empty launch
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    stacked = [_dev(np.stack(part), hip_device) for part in (regimes, means, covs, noise)]
    with pytest.raises(ValueError, match="regimes must be"):
        provider.switching_state_draw(ops, stacked[0].to(torch.int64), *stacked[1:])
    with pytest.raises(ValueError, match="noise must be"):
        provider.switching_state_draw(ops, stacked[0], stacked[1], stacked[2], stacked[3][:, :, :, :2])
    with pytest.raises(ValueError, match="z_next must be"):
        provider.switching_state_draw(ops, *stacked, following=(stacked[0][0], stacked[1][0][:, :5]))
    empty = provider.switching_state_draw(ops, *[part[:, :, :0] for part in stacked])
    assert empty.shape == (T, B, 0, D) and provider.read_flags(hip_device) == 0


def test_the_function_end_to_end(hip_device):
    """`switching_sample_states` on the device: replayed noise gives the same bits, fresh noise differs between calls and
    replays, an out-of-range regime is ONE ValueError at the end and leaves the flags clean."""
    from aesmc_amd import rao_blackwell
    provider = _provider()
    M, D, Dy, B, N, T = 3, 2, 2, 2, 65, 5
    model, regimes, observations, noise = _case(M, D, Dy, B, N, T, seed=2)
    slg = _torch_model(model, hip_device)
    ys, paths = [_dev(y, hip_device) for y in observations], [_dev(regime, hip_device) for regime in regimes]
    given = [_dev(eps, hip_device) for eps in noise]
    first = rao_blackwell.switching_sample_states(ys, slg, paths, noise=given)
    second = rao_blackwell.switching_sample_states(ys, slg, paths, noise=given)
    assert all(torch.equal(a, b) for a, b in zip(first["states"], second["states"]))
    assert len(first["states"]) == T and all(z.shape == (B, N, D) and z.dtype == torch.float64 for z in first["states"])
    want = draw.state_draw_pass(model, regimes, observations, noise)
    filtered = rao_blackwell.conditional_kalman_filter(ys, slg, paths)
    assert torch.equal(first["log_likelihood"], filtered["log_likelihood"])
    for t in range(T):      # (the device's own filtered moments: a loose sanity bound; the sharp one is the kernel test's)
        np.testing.assert_allclose(first["states"][t].cpu().numpy(), want["states"][t], rtol=0, atol=1e-10)
    fresh, other = rao_blackwell.switching_sample_states(ys, slg, paths), rao_blackwell.switching_sample_states(ys, slg, paths)
    assert not torch.equal(fresh["states"][0], other["states"][0]) and not torch.equal(fresh["noise"][0], other["noise"][0])
    replay = rao_blackwell.switching_sample_states(ys, slg, paths, noise=fresh["noise"])
    assert all(torch.equal(a, b) for a, b in zip(fresh["states"], replay["states"]))
    bad = [path.clone() for path in paths]
    bad[2][1, 64] = M
    with pytest.raises(ValueError, match="regimes holds a value outside"):
        rao_blackwell.switching_sample_states(ys, slg, bad, noise=given)
    assert provider.read_flags(hip_device) == 0
    again = rao_blackwell.switching_sample_states(ys, slg, paths, noise=given)
    assert all(torch.equal(a, b) for a, b in zip(first["states"], again["states"]))
