"""The smoothed continuous state of switching linear-Gaussian models on the device: kernel K36
(aesmc_switching_smooth_combine) against its NumPy contract (aesmc_amd/testing/rao_blackwell.py) within the contract's bound,
its conventions, the C ABI's refusals, and `aesmc_amd.rao_blackwell.conditional_kalman_filter`, `switching_state_smooth` and
`switching_smooth_states` end to end: replayed against the contract's pass within its propagated tolerances, the one-regime
case against the dense Gaussian conditioning, and statistically against the enumeration of all regime sequences."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

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


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


def _device_combine(provider, device, model, regime_next, filtered, factor, lam, omega_next, cov_next, cross=True):
    ops = {name: _dev(value, device) for name, value in model.items()} if cross else None
    out = provider.switching_smooth_combine(ops, _dev(regime_next, device) if cross else None,
                                            tuple(_dev(part, device) for part in filtered), _dev(factor, device),
                                            _dev(lam, device), _dev(omega_next, device) if cross else None,
                                            _dev(cov_next, device) if cross else None)
    return [None if part is None else part.cpu().numpy() for part in out]


@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("steps", [1, 2, 3])      # omega_next NULL; a rank-deficient Om handed over where Dy < D; a later one
@pytest.mark.parametrize("B,K,N,M,D,Dy", contract.BACKWARD_SHAPES)
def test_the_combination_equals_the_contract_within_its_bound(hip_device, B, K, N, M, D, Dy, steps, cross):
    provider = _provider()
    args = contract.example_smooth_combine(B, N, M, D, Dy, steps=steps)
    got = _device_combine(provider, hip_device, *args, cross=cross)
    assert provider.read_flags(hip_device) == 0
    if not cross:
        args = (None, None) + args[2:5] + (None, None)
    want = contract.switching_smooth_combine(*args)
    bounds = contract.switching_smooth_combine_bound(*args)
    assert want[3] == 0 and (got[2] is None) == (not cross)
    for name, part, expected, bound, tail in zip(("mean", "cov", "cross"), got, want[:3], bounds,
                                                 ((D,), (D * (D + 1) // 2,), (D, D))):
        if part is None:
            continue
        assert part.shape == (B, N) + tail and part.dtype == np.float64, name
        error = np.abs(part - expected)
        print(name, "largest error", error.max(), "of bound", (error / np.where(bound > 0, bound, 1.0)).max())
        assert (error <= bound).all(), name


def test_regimes_out_of_range_singular_noise_and_a_zero_covariance(hip_device):
    provider = _provider()
    B, N, M, D, Dy = 2, 300, 4, 5, 3
    args = list(contract.example_smooth_combine(B, N, M, D, Dy, steps=2))
    clean = _device_combine(provider, hip_device, *args)
    assert provider.read_flags(hip_device) == 0
    # a regime outside [0, M): NaN in that trajectory's three outputs only, and the flag
    bad = args[1].copy()
    bad[1, 299], bad[0, 3], bad[1, 256] = M, -1, 1 << 20
    gone = np.zeros((B, N), dtype=bool)
    gone[1, 299] = gone[0, 3] = gone[1, 256] = True
    got = _device_combine(provider, hip_device, args[0], bad, *args[2:])
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    for part, reference in zip(got, clean):
        assert np.isnan(part[gone]).all() and np.array_equal(part[~gone], reference[~gone])
    # ... which nothing reads without the cross-covariance
    got = _device_combine(provider, hip_device, args[0], bad, *args[2:], cross=False)
    assert provider.read_flags(hip_device) == 0 and got[2] is None
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # q = 0 in the regimes' noise and P = 0: finite, within the bound
    model = dict(args[0], q=np.zeros_like(args[0]["q"]))
    zero = (args[2][0], np.zeros_like(args[2][1]))
    for case in ((model, args[1], args[2]), (args[0], args[1], zero), (model, args[1], zero)):
        operands = case + tuple(args[3:])
        got = _device_combine(provider, hip_device, *operands)
        want = contract.switching_smooth_combine(*operands)
        bounds = contract.switching_smooth_combine_bound(*operands)
        assert provider.read_flags(hip_device) == 0
        for part, expected, bound in zip(got, want[:3], bounds):
            assert np.isfinite(part).all() and (np.abs(part - expected) <= bound).all()
    assert (got[1] == 0).all() and np.array_equal(got[0], args[2][0])      # P = 0: nothing to learn, m^s = m, P^s = 0


def test_the_abi_refuses_bad_arguments_without_a_launch(hip_device):
    """Device pointers this time: a refusal must leave the outputs as they were."""
    from aesmc_amd import _lib
    lib = _lib.load()
    B, N, M, D, Dy = 2, 5, 2, 2, 1
    model, regime_next, filtered, factor, lam, omega_next, cov_next = contract.example_smooth_combine(B, N, M, D, Dy, steps=2)
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    keys = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    block = lambda **kw: _lib.SwitchingModel(*([ops[name].data_ptr() for name in keys] + [kw.get("M", M), kw.get("D", D),
                                                                                          kw.get("Dy", Dy)]))
    dev = [_dev(part, hip_device) for part in (regime_next,) + filtered + (factor, lam, omega_next, cov_next)]
    outs = [torch.full(shape, 7.0, dtype=torch.float64, device=hip_device) for shape in ((B, N, D), (B, N, 3), (B, N, D, D))]
    ptr = lambda t: None if t is None else t.data_ptr()

    def combine(model="default", inputs=dev, outputs=outs, B=B, N=N, D=D):
        model = block() if model == "default" else model
        return lib.aesmc_switching_smooth_combine(None if model is None else ctypes.byref(model), *[ptr(t) for t in inputs],
                                                  *[ptr(t) for t in outputs], None, B, N, D, None)

    assert combine(inputs=dev[:1] + [None] + dev[2:]) == 1 and combine(outputs=[None] + outs[1:]) == 1
    assert combine(model=None) == 1 and combine(inputs=[None] + dev[1:]) == 1 and combine(outputs=outs[:2] + [None]) == 1
    assert combine(outputs=[dev[1]] + outs[1:]) == 1 and combine(outputs=outs[:2] + [outs[1]]) == 1 and combine(B=-1) == 1
    assert combine(model=block(D=3)) == 1
    assert combine(model=block(D=9), D=9) == 2 and combine(model=block(M=17)) == 2 and combine(B=1 << 16, N=1 << 16) == 2
    assert combine(B=0) == 0 and combine(N=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)


def _norms(error_means, error_covs, D):
    return (float(np.linalg.norm(error_means, axis=-1).max()),
            float(np.linalg.norm(contract.unpack(error_covs, D), 2, axis=(-2, -1)).max()))


@pytest.mark.parametrize("observation_dtype", [torch.float64, torch.float32])
def test_the_filter_and_the_smoother_along_given_regimes_equal_the_contracts_pass(hip_device, observation_dtype):
    """`conditional_kalman_filter` and `switching_state_smooth` on the device, every launch fed what the device itself wrote,
    against `switching_state_pass` within the tolerances it propagates (the Euclidean norm of a trajectory's mean error, the
    spectral norm of its covariance and cross-covariance errors)."""
    from aesmc_amd import rao_blackwell
    T, B, N, M, D, Dy = 5, 3, 7, 3, 2, 2
    ops = contract.example_model(M, D, Dy, seed=5)
    model = _torch_model(ops, hip_device)
    observations = [y.to(observation_dtype) for y in model.simulate(T, B, seed=3)]
    rng = np.random.default_rng(9)
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    paths = [_dev(regime, hip_device) for regime in regimes]
    want = contract.switching_state_pass(ops, regimes, [y.cpu().numpy() for y in observations])
    tolerances = want["tolerances"]
    assert want["flags"] == 0 and min(want["pivot_margins"]) > 1e-13
    filtered = rao_blackwell.conditional_kalman_filter(observations, model, paths)
    out = rao_blackwell.switching_state_smooth(observations, model, paths, return_cross_moments=True, return_trajectories=True)
    worst = 0.0
    for result in (filtered, out):
        error = np.abs(result["log_likelihood"].cpu().numpy() - want["log_likelihood"]).max()
        worst = max(worst, error / tolerances["log_likelihood"])
        assert error <= tolerances["log_likelihood"]
    for t in range(T):
        error_m, error_p = _norms(filtered["means"][t].cpu().numpy() - want["filtered_means"][t],
                                  filtered["covariances"][t].cpu().numpy() - want["filtered_covariances"][t], D)
        worst = max(worst, error_m / tolerances["filtered_means"][t], error_p / tolerances["filtered_covariances"][t])
        assert error_m <= tolerances["filtered_means"][t] and error_p <= tolerances["filtered_covariances"][t], t
        error_m, error_p = _norms(out["means"][t].cpu().numpy() - want["means"][t],
                                  out["covariances"][t].cpu().numpy() - want["covariances"][t], D)
        worst = max(worst, error_m / tolerances["means"][t], error_p / tolerances["covariances"][t])
        assert error_m <= tolerances["means"][t] and error_p <= tolerances["covariances"][t], t
        if t < T - 1:
            error_x = float(np.linalg.norm(out["cross_covariances"][t].cpu().numpy() - want["cross_covariances"][t], 2,
                                           axis=(-2, -1)).max())
            worst = max(worst, error_x / tolerances["cross_covariances"][t])
            assert error_x <= tolerances["cross_covariances"][t], t
    print("largest device error over propagated tolerance", worst)
    means = np.stack(want["means"])
    average = means.mean(axis=2)
    second = (contract.unpack(np.stack(want["covariances"]), D) + means[..., :, None] * means[..., None, :]).mean(axis=2)
    lagged = (np.stack(want["cross_covariances"]) + means[1:, ..., :, None] * means[:-1, ..., None, :]).mean(axis=2)
    # the moments: a covariance within tol_P plus products m m^T of values within tol_m, twice (the second moment and the
    # square of the average), and the rounding of N + 4 operations on values of size |m|^2
    size = np.abs(means).max()
    loosest = max(max(tolerances[key]) for key in ("means", "covariances", "cross_covariances"))
    atol = (1.0 + 4.0 * size) * loosest + (N + 4) * contract.UNIT * (1.0 + size * size)
    np.testing.assert_allclose(out["smoothed_mean"].cpu().numpy(), average, rtol=0, atol=atol)
    np.testing.assert_allclose(out["smoothed_covariance"].cpu().numpy(),
                               second - average[..., :, None] * average[..., None, :], rtol=0, atol=atol)
    np.testing.assert_allclose(out["smoothed_cross_moment"].cpu().numpy(), lagged, rtol=0, atol=atol)
    # a regime outside [0, M) is reported at the end, and nothing stays flagged
    paths[2] = paths[2].clone()
    paths[2][1, 4] = M
    with pytest.raises(ValueError, match="regimes holds a value outside"):
        rao_blackwell.switching_state_smooth(observations, model, paths, return_cross_moments=True)
    assert _provider().read_flags(hip_device) == 0


@pytest.mark.parametrize("K,N", [(1, 1), (33, 300)])
def test_one_regime_is_the_exact_smoother_on_the_device(hip_device, K, N):
    """With M = 1 nothing is sampled: `switching_smooth_states` against `exact_state_smoother` within the pass's propagated
    tolerances and nothing else, for any K and N."""
    from aesmc_amd import rao_blackwell
    T, B, D, Dy = 5, 2, 3, 2
    ops = contract.example_model(1, D, Dy, seed=7)
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=2)
    ys = [y.cpu().numpy() for y in observations]
    out, log_z = rao_blackwell.switching_smooth_states(observations, model, K, num_trajectories=N)
    tolerances = contract.switching_state_pass(ops, [np.zeros((B, 1), dtype=np.int32)] * T, ys)["tolerances"]
    worst = 0.0
    for b in range(B):
        means, covs, crosses = contract.exact_state_smoother(ops, (0,) * T, [y[b] for y in ys])
        lagged = crosses + means[1:, :, None] * means[:-1, None, :]
        pairs = []
        for t in range(T):
            pairs.append((out["smoothed_mean"][t, b], means[t], tolerances["means"][t]))
            # (the mixture's covariance and cross moment: products of means within tol_m beside the trajectories' own)
            pairs.append((out["smoothed_covariance"][t, b], covs[t],
                          tolerances["covariances"][t] + 4 * np.abs(means[t]).max() * tolerances["means"][t]))
            if t < T - 1:
                reach = np.abs(means).max() * (tolerances["means"][t] + tolerances["means"][t + 1])
                pairs.append((out["smoothed_cross_moment"][t, b], lagged[t], tolerances["cross_covariances"][t] + 2 * reach))
        exact = contract.exact_log_likelihood(ops, [y[b] for y in ys])
        # (the evidence: `switching_pass`'s (K + 4) u (1 + |lse| + log K) per step beside the summed log-weights' tolerance)
        pairs.append((log_z[b], exact, tolerances["log_likelihood"] +
                      T * (K + 4) * contract.UNIT * (1.0 + abs(exact) + np.log(K))))
        pairs.append((out["log_likelihood"][b], exact, tolerances["log_likelihood"]))
        for got, want, tolerance in pairs:
            worst = max(worst, float((np.abs(got.cpu().numpy() - want) / tolerance).max()))
    print("largest error over the propagated tolerance", worst)
    assert worst <= 1.0


def test_every_documented_key_after_both_filters(hip_device):
    from aesmc_amd import rao_blackwell
    T, B, K, N, M, D, Dy = 4, 3, 65, 17, 3, 8, 8
    TD = D * (D + 1) // 2
    model = _torch_model(contract.example_model(M, D, Dy, seed=2), hip_device)
    observations = model.simulate(T, B, seed=4)
    for lookahead in (False, True):
        out, log_z = rao_blackwell.switching_smooth_states(observations, model, K, num_trajectories=N, lookahead=lookahead,
                                                           return_trajectories=True)
        assert sorted(out) == ["covariances", "cross_covariances", "log_likelihood", "means", "regimes", "smoothed_covariance",
                               "smoothed_cross_moment", "smoothed_mean", "smoothed_regime_probabilities"]
        assert log_z.shape == (B,) and out["log_likelihood"].shape == (B, N)
        assert out["smoothed_mean"].shape == (T, B, D) and out["smoothed_covariance"].shape == (T, B, D, D)
        assert out["smoothed_cross_moment"].shape == (T - 1, B, D, D) and out["smoothed_regime_probabilities"].shape == (T, B, M)
        assert [r.shape for r in out["regimes"]] == [(B, N)] * T and all(r.dtype == torch.int32 for r in out["regimes"])
        assert [m.shape for m in out["means"]] == [(B, N, D)] * T and [c.shape for c in out["covariances"]] == [(B, N, TD)] * T
        assert [x.shape for x in out["cross_covariances"]] == [(B, N, D, D)] * (T - 1)
        for key in ("smoothed_mean", "smoothed_covariance", "smoothed_cross_moment", "log_likelihood"):
            assert out[key].dtype == torch.float64 and bool(torch.isfinite(out[key]).all()), key
        assert bool((torch.linalg.eigvalsh(out["smoothed_covariance"]) > -1e-12).all())
        plain, _ = rao_blackwell.switching_smooth(observations, model, K, num_trajectories=N, lookahead=lookahead)
        assert sorted(plain) == ["regimes", "smoothed_regime_probabilities"]


def test_the_smoothed_mean_on_the_device_against_the_enumeration(hip_device):
    """The CPU file's statistical check with fresh device uniforms, after both filters: one series copied to B = 64 rows,
    K = N = 256; the row-mean of smoothed_mean within 4 across-row standard errors plus spread / K of the exact E[z_t | y],
    and closer to it in summed absolute error than the row-mean of the filtered means."""
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(2, 2, 1, seed=4)
    model = _torch_model(ops, hip_device)
    series = [y[0].cpu().numpy() for y in _torch_model(ops, "cpu").simulate(6, 1, seed=9)]
    exact, _, _ = contract.exact_smoothed_state(ops, series)
    spread = max(float(np.abs(contract.exact_state_smoother(ops, sequence, series)[0] - exact).max())
                 for sequence in itertools.product(range(2), repeat=6))
    B, K, N = 64, 256, 256
    observations = [_dev(np.broadcast_to(y, (B, 1)).copy(), hip_device) for y in series]
    torch.manual_seed(23)
    np.random.seed(23)
    for lookahead in (False, True):
        run = rao_blackwell.adapted_switching_filter if lookahead else rao_blackwell.switching_filter
        filtered = run(observations, model, K, resampling="systematic", return_moments=True)
        drawn = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N)
        out = rao_blackwell.switching_state_smooth(observations, model, drawn["regimes"])
        smoothed = out["smoothed_mean"].cpu().numpy()
        mean, standard_error = smoothed.mean(axis=1), smoothed.std(axis=1, ddof=1) / np.sqrt(B)
        error, allowance = np.abs(mean - exact), 4 * standard_error + spread / K
        filtered_error = np.abs(filtered["filtered_mean"].cpu().numpy().mean(axis=1) - exact)
        print("lookahead", lookahead, "spread", spread, "largest error", error.max(), "largest ratio",
              (error / allowance).max(), "summed: smoothed", error.sum(), "filtered", filtered_error.sum())
        assert (error <= allowance).all()
        assert error.sum() < filtered_error.sum()
