"""Rao-Blackwellised backward simulation for switching linear-Gaussian models on the device: kernels K34
(aesmc_switching_information_step) and K35 (aesmc_switching_backward_scores) against their NumPy contract
(aesmc_amd/testing/rao_blackwell.py) within the contract's bounds, their conventions, the C ABI's refusals, and
`aesmc_amd.rao_blackwell.switching_backward_simulate` end to end: replayed against the contract's pass after both filters,
statistically against the enumeration of all regime sequences, and on a trajectory nothing can precede."""
import ctypes

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


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


def _device_information(provider, device, model, regime_next, info, y):
    ops = {name: _dev(value, device) for name, value in model.items()}
    out = provider.switching_information_step(ops, _dev(regime_next, device),
                                              None if info is None else tuple(_dev(part, device) for part in info),
                                              _dev(y, device))
    return [part.cpu().numpy() for part in out]


def _device_scores(provider, device, log_Pi, regime_next, factor, lam, particles, log_w):
    return provider.switching_backward_scores(_dev(log_Pi, device), _dev(regime_next, device), _dev(factor, device),
                                              _dev(lam, device), tuple(_dev(part, device) for part in particles),
                                              _dev(log_w, device)).cpu().numpy()


class _Replay:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


@pytest.mark.parametrize("observation_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("steps", [1, 2, 3])      # the first (NULL) step; a rank-deficient Om handed over where Dy < D; a later one
@pytest.mark.parametrize("B,K,N,M,D,Dy", contract.BACKWARD_SHAPES)
def test_information_step_and_scores_equal_the_contract_within_its_bounds(hip_device, B, K, N, M, D, Dy, steps,
                                                                          observation_dtype):
    provider = _provider()
    model, regime_next, info, y, particles, log_w = contract.example_backward_step(B, K, N, M, D, Dy, steps=steps,
                                                                                   observation_dtype=observation_dtype)
    TD = D * (D + 1) // 2
    got = _device_information(provider, hip_device, model, regime_next, info, y)
    assert provider.read_flags(hip_device) == 0
    want = contract.switching_information_step(model, regime_next, info, y)
    bounds = contract.switching_information_step_bound(model, regime_next, info, y)
    assert want[4] == 0 and want[5] > 1e-13      # no pivot near the threshold: the device keeps and drops the same columns
    if steps == 2 and Dy < D:
        assert np.linalg.matrix_rank(contract.unpack(info[0], D)[0, 0], tol=1e-9) == Dy
    for name, part, expected, bound, shape in zip(("Om", "lam", "c", "F"), got, want[:4], bounds,
                                                  ((B, N, TD), (B, N, D), (B, N), (B, N, TD))):
        assert part.shape == shape and part.dtype == np.float64, name
        error = np.abs(part - expected)
        print(name, "largest error", error.max(), "of bound", (error / np.where(bound > 0, bound, 1.0)).max())
        assert (error <= bound).all(), name
    assert np.array_equal(got[3] == 0, want[3] == 0)
    log_Pi = _log(model["Pi"])
    for weights in (log_w, None):
        scores = _device_scores(provider, hip_device, log_Pi, regime_next, want[3], want[1], particles, weights)
        assert provider.read_flags(hip_device) == 0 and scores.shape == (B, N, K) and scores.dtype == np.float64
        expected, _ = contract.switching_backward_scores(log_Pi, regime_next, want[3], want[1], particles, weights)
        bound = contract.switching_backward_scores_bound(log_Pi, regime_next, want[3], want[1], particles, weights)
        error = np.abs(scores - expected)
        print("scores: largest error", error.max(), "of bound", (error / bound).max())
        assert (error <= bound).all()


def test_zero_transition_probabilities_and_regimes_out_of_range(hip_device):
    provider = _provider()
    B, K, N, M, D, Dy = 2, 300, 17, 4, 5, 3
    model, regime_next, info, y, particles, log_w = contract.example_backward_step(B, K, N, M, D, Dy, steps=2)
    om, lam, c, F, _, _ = contract.switching_information_step(model, regime_next, info, y)
    log_Pi = _log(model["Pi"])
    clean = _device_scores(provider, hip_device, log_Pi, regime_next, F, lam, particles, log_w)
    assert provider.read_flags(hip_device) == 0
    # a zero transition probability: -inf and not NaN, also where the particle's weight is NaN
    blocked = log_Pi.copy()
    blocked[1, 2] = blocked[3, 0] = -np.inf
    poisoned = log_w.copy()
    poisoned[0, 0] = np.nan
    got = _device_scores(provider, hip_device, blocked, regime_next, F, lam, particles, poisoned)
    want, _ = contract.switching_backward_scores(blocked, regime_next, F, lam, particles, poisoned)
    assert provider.read_flags(hip_device) == 0
    excluded = np.isneginf(want)
    assert excluded.any() and np.isneginf(got[excluded]).all() and not np.isneginf(got[~excluded]).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == N - excluded[0, :, 0].sum()
    rest = ~excluded & ~np.isnan(want)
    assert np.array_equal(got[rest], clean[rest])
    # a regime outside [0, M) on either side: NaN there only, and the flag
    bad_next, bad_regime = regime_next.copy(), particles[0].copy()
    bad_next[1, 16], bad_next[0, 3], bad_regime[0, 4], bad_regime[1, 299] = M, -1, -1, 1 << 20
    dead = np.zeros((B, N, K), dtype=bool)
    dead[1, 16, :] = dead[0, 3, :] = dead[0, :, 4] = dead[1, :, 299] = True
    got = _device_scores(provider, hip_device, log_Pi, bad_next, F, lam, (bad_regime, particles[1], particles[2]), log_w)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    assert np.isnan(got[dead]).all() and np.array_equal(got[~dead], clean[~dead])
    reference = _device_information(provider, hip_device, model, regime_next, info, y)
    assert provider.read_flags(hip_device) == 0
    got = _device_information(provider, hip_device, model, bad_next, info, y)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    gone = np.zeros((B, N), dtype=bool)
    gone[1, 16] = gone[0, 3] = True
    for part, expected in zip(got, reference):
        assert np.isnan(part[gone]).all() and np.array_equal(part[~gone], expected[~gone])


def test_the_abi_refuses_bad_arguments_without_a_launch(hip_device):
    """Device pointers this time: a refusal must leave the outputs as they were."""
    from aesmc_amd import _lib
    lib = _lib.load()
    B, K, N, M, D, Dy = 2, 7, 5, 2, 2, 1
    model, regime_next, info, y, particles, log_w = contract.example_backward_step(B, K, N, M, D, Dy, steps=2)
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    keys = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    block = lambda **kw: _lib.SwitchingModel(*([ops[name].data_ptr() for name in keys] + [kw.get("M", M), kw.get("D", D),
                                                                                          kw.get("Dy", Dy)]))
    dev = [_dev(part, hip_device) for part in (regime_next,) + info + (y,)]
    outs = [torch.full(shape, 7.0, dtype=torch.float64, device=hip_device) for shape in ((B, N, 3), (B, N, 2), (B, N), (B, N, 3))]
    ptr = lambda t: None if t is None else t.data_ptr()

    def step(model=None, inputs=dev, outputs=outs, B=B, N=N, dtype=1):
        model = block() if model is None else model
        return lib.aesmc_switching_information_step(dtype, ctypes.byref(model), *[ptr(t) for t in inputs],
                                                     *[ptr(t) for t in outputs], None, B, N, None)

    assert step(inputs=[None] + dev[1:]) == 1 and step(inputs=dev[:1] + [None] + dev[2:]) == 1
    assert step(outputs=outs[:3] + [None]) == 1 and step(outputs=[dev[1]] + outs[1:]) == 1 and step(dtype=5) == 1
    assert step(outputs=outs[:3] + [outs[0]]) == 1 and step(B=-1) == 1
    assert step(model=block(D=9)) == 2 and step(model=block(M=17)) == 2 and step(B=1 << 16, N=1 << 16) == 2
    assert step(B=0) == 0 and step(N=0) == 0
    state = [_dev(part, hip_device) for part in particles]
    traj = [_dev(_log(model["Pi"]), hip_device), dev[0], outs[3], outs[1]]
    scores = torch.full((B, N, K), 7.0, dtype=torch.float64, device=hip_device)

    def score(operands=traj + state + [_dev(log_w, hip_device)], out=scores, B=B, K=K, N=N, M=M, D=D):
        return lib.aesmc_switching_backward_scores(*[ptr(t) for t in operands], ptr(out), None, B, K, N, M, D, None)

    assert score(operands=[None] + traj[1:] + state + [None]) == 1 and score(out=None) == 1 and score(out=state[1]) == 1
    assert score(K=-1) == 1 and score(M=0) == 1 and score(D=0) == 1
    assert score(D=9) == 2 and score(M=17) == 2 and score(B=1 << 11, K=1 << 10, N=1 << 10) == 2
    assert score(B=0) == 0 and score(K=0) == 0 and score(N=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [scores])


@pytest.mark.parametrize("adapted", [False, True])
@pytest.mark.parametrize("B,K,N,M,D,Dy,seed", [(2, 300, 17, 4, 5, 3, 0), (3, 65, 64, 3, 8, 8, 0)])
def test_backward_simulation_on_replayed_uniforms_equals_the_contracts_pass(hip_device, B, K, N, M, D, Dy, seed, adapted):
    """The filter runs on the device; the contract's backward pass runs on what the device stored, with the same uniforms.
    Every index is equal, except draws whose contract margin (the distance of u from the nearest step of the normalised
    running sum) is within what scores off by their bounds can move that sum: a score off by e scales its weight by
    exp(+-e), a normalised partial sum by at most exp(2 e) - 1 <= 4 e — with e the bounds of this step and of the steps
    before it in the trajectory (later in time) summed.  A trajectory excused once is excused from there on (it walks
    another path).  The excused draws may be at most 0.1 % of all; with float64 scores the expected number is zero."""
    from aesmc_amd import inference, rao_blackwell
    T = 5
    ops = contract.example_model(M, D, Dy, seed)
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=seed + 1)
    rng = np.random.default_rng([seed, 78])
    regime_u, resample_u = [rng.uniform(size=(B, K)) for _ in range(T)], [rng.uniform(size=B) for _ in range(T - 1)]
    uniforms = [rng.uniform(size=(B, N)) for _ in range(T)]
    run = rao_blackwell.adapted_switching_filter if adapted else rao_blackwell.switching_filter
    with inference.uniform_feed(_Replay([_dev(u, hip_device) for u in resample_u])):
        filtered = run(observations, model, K, resampling="systematic", regime_uniforms=[_dev(u, hip_device) for u in regime_u])
    out = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N,
                                                    uniforms=[_dev(u, hip_device) for u in uniforms], return_indices=True)
    keys = ("regimes", "means", "covariances") + (() if adapted else ("log_weights",))
    stored = {key: [part.cpu().numpy() for part in filtered[key]] for key in keys}
    want = contract.switching_backward_pass(stored, ops, [y.cpu().numpy() for y in observations], uniforms)
    assert want["flags"] == 0 and min(want["pivot_margins"]) > 1e-13
    excused = np.zeros((B, N), dtype=bool)
    carried = np.zeros((B, N))
    count = 0
    for t in range(T - 1, -1, -1):
        carried = carried + want["score_bounds"][t]
        excused |= want["margins"][t] <= 4.0 * carried
        count += int(excused.sum())
        index, regime = out["indices"][t].cpu().numpy(), out["regimes"][t].cpu().numpy()
        assert index.dtype == np.int64 and regime.dtype == np.int32 and index.shape == regime.shape == (B, N)
        differs = (index != want["indices"][t]) | (regime != want["regimes"][t])
        assert not (differs & ~excused).any(), t
        excused |= differs
    print("excused draws", count, "of", T * B * N, "smallest margin", min(float(m.min()) for m in want["margins"]))
    assert count <= 0.001 * T * B * N
    frequencies = np.stack([np.stack([(r.cpu().numpy() == i).mean(axis=1) for i in range(M)], axis=1) for r in out["regimes"]])
    np.testing.assert_allclose(out["smoothed_regime_probabilities"].cpu().numpy(), frequencies, rtol=0, atol=1e-15)


@pytest.mark.parametrize("M,D,Dy", [(3, 8, 8), (4, 5, 3), (2, 2, 1)])
def test_information_over_a_time_series_stays_within_the_propagated_bounds(hip_device, M, D, Dy):
    """K34 chained over T = 12 steps along given regime paths, every step fed what the device itself wrote: the distance
    from the contract's chain in Om (spectral norm) and lam (Euclidean norm) against the tolerances the contract propagates
    (`switching_information_pass`).  The largest ratio is the figure DESIGN.md section 22 quotes."""
    provider = _provider()
    T, B, N = 12, 2, 33
    ops = contract.example_model(M, D, Dy, seed=2)
    rng = np.random.default_rng([M, D, Dy, 35])
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    ys = [rng.standard_normal((B, Dy)) for _ in range(T)]
    want = contract.switching_information_pass(ops, regimes, ys)
    assert want["flags"] == 0 and min(want["pivot_margins"]) > 1e-13
    device_ops = {name: _dev(value, hip_device) for name, value in ops.items()}
    info, worst = None, 0.0
    for t in range(T - 2, -1, -1):
        om, lam, c, factor = provider.switching_information_step(device_ops, _dev(regimes[t + 1], hip_device), info,
                                                                 _dev(ys[t + 1], hip_device))
        info = (om, lam, c)
        expected = want["information"][t]
        error_o = np.linalg.norm(contract.unpack(om.cpu().numpy() - expected[0], D), 2, axis=(-2, -1)).max()
        error_l = np.linalg.norm(lam.cpu().numpy() - expected[1], axis=-1).max()
        tol_o, tol_l = want["tolerances"]["omega"][t], want["tolerances"]["lambda"][t]
        worst = max(worst, error_o / tol_o, error_l / tol_l)
        assert error_o <= tol_o and error_l <= tol_l, t
    assert provider.read_flags(hip_device) == 0
    print("largest device error over propagated tolerance", worst)


def test_smoothed_probabilities_on_the_device_against_the_enumeration(hip_device):
    """The CPU file's statistical check with fresh device uniforms: one series copied to B = 64 rows, K = 256, N = 256; the
    row-mean of the smoothed regime probabilities within 4 across-row standard errors plus 1/K of the exact smoothed
    marginals, and closer to them in summed absolute error than the row-mean of the filtered ones."""
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(2, 2, 1, seed=4)
    model = _torch_model(ops, hip_device)
    series = [y[0].cpu().numpy() for y in _torch_model(ops, "cpu").simulate(6, 1, seed=9)]
    exact = contract.exact_regime_marginals(ops, series)
    B, K, N = 64, 256, 256
    observations = [_dev(np.broadcast_to(y, (B, 1)).copy(), hip_device) for y in series]
    torch.manual_seed(23)
    np.random.seed(23)
    for lookahead in (False, True):
        run = rao_blackwell.adapted_switching_filter if lookahead else rao_blackwell.switching_filter
        filtered = run(observations, model, K, resampling="systematic", return_moments=True)
        out = rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=N)
        smoothed = out["smoothed_regime_probabilities"].cpu().numpy()
        mean, standard_error = smoothed.mean(axis=1), smoothed.std(axis=1, ddof=1) / np.sqrt(B)
        error = np.abs(mean - exact)
        filtered_error = np.abs(filtered["regime_probabilities"].cpu().numpy().mean(axis=1) - exact)
        print("lookahead", lookahead, "largest error", error.max(), "largest ratio",
              (error / (4 * standard_error + 1.0 / K)).max(), "summed: smoothed", error.sum(), "filtered", filtered_error.sum())
        assert (error <= 4 * standard_error + 1.0 / K).all()
        assert error.sum() < filtered_error.sum()


def test_a_trajectory_nothing_can_precede_raises(hip_device):
    """Regime 1 cannot be entered, yet every stored particle of the last step is made to sit there: the scores of step T-2
    are a row of -inf per trajectory, and the one read of the flags at the end raises `backward_simulate`'s RuntimeError."""
    from aesmc_amd import rao_blackwell
    T, B, K = 3, 2, 40
    ops = contract.example_model(2, 2, 1, seed=6)
    ops = contract.operands(np.array([1.0, 0.0]), np.array([[1.0, 0.0], [1.0, 0.0]]), *[ops[name] for name in MODEL_KEYS[2:]])
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=1)
    filtered = rao_blackwell.switching_filter(observations, model, K)
    filtered = dict(filtered, regimes=filtered["regimes"][:-1] + [torch.ones_like(filtered["regimes"][-1])])
    with pytest.raises(RuntimeError, match="no finite maximum"):
        rao_blackwell.switching_backward_simulate(filtered, model, observations, num_trajectories=9)
    assert _provider().read_flags(hip_device) == 0
    # ... and the same systems smooth fine as they were stored
    out, log_z = rao_blackwell.switching_smooth(observations, model, K, num_trajectories=9)
    assert all((r == 0).all() for r in out["regimes"]) and torch.isfinite(log_z).all()
