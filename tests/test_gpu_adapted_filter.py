"""The fully adapted auxiliary particle filter on the device: kernels K27 (aesmc_affine_quadratic_logweight) and K28
(aesmc_adapted_draw) against their NumPy contracts (aesmc_amd/testing/adapted.py) within the contracts' bounds, their
views, the out-of-range convention, and `aesmc_amd.adapted.adapted_filter` end to end: replayed against the restated
filter in float64, against the Kalman filter, statistically against `infer("smc")` with the transition as proposal, and
handed on to the smoothers."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as contract

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (3, 7, 2, 3), (2, 65, 3, 2), (2, 300, 10, 10), (1, 1025, 16, 16), (2, 257, 16, 1)]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _operands(B, K, D, Dy, dtype, seed):
    rng = np.random.RandomState(seed)
    gain = contract.gains(0.5 + rng.rand(D), np.eye(Dy, D) + 0.3 * rng.randn(Dy, D), 0.3 + rng.rand(Dy))
    o, r = contract.row_offsets(gain, rng.randn(B, Dy))
    loc = (2.0 * rng.randn(B, K, D)).astype(dtype)
    eps = rng.randn(B, K, D).astype(dtype)
    return gain, o, r, loc, eps


def _device_loc(loc, layout, device):
    """`loc` on the device: dense, or (layout 'row') its first particle read with particle stride 0."""
    t = torch.from_numpy(loc).to(device)
    if layout == "row":
        return t[:, :1].contiguous().expand(loc.shape), np.broadcast_to(loc[:, :1], loc.shape)
    return t, loc


def _within(got, want, bound, dtype):
    """float64: within the contract's bound; float32: within one unit in the last place of float32."""
    if dtype == np.float64:
        return np.abs(got - want) <= bound
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("layout", ["dense", "row"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D,Dy", SHAPES)
def test_quadratic_logweight_equals_contract(hip_device, B, K, D, Dy, dtype, layout):
    provider = _provider()
    gain, o, _, loc, _ = _operands(B, K, D, Dy, dtype, 7 * K + D)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    device_loc, host_loc = _device_loc(loc, layout, hip_device)
    out = provider.affine_quadratic_logweight(device_loc, dev(gain["P"]), dev(o), gain["base"])
    assert out.dtype == TORCH[dtype] and tuple(out.shape) == (B, K)
    want = contract.affine_quadratic_logweight(host_loc, gain["P"], o, gain["base"])
    bound = contract.affine_quadratic_logweight_bound(host_loc, gain["P"], o, gain["base"])
    ok = _within(out.cpu().numpy(), want, bound, dtype)
    assert ok.all(), (np.argwhere(~ok)[:4], np.abs(out.cpu().numpy() - want).max(), bound.max())
    assert provider.read_flags(hip_device) == 0


@pytest.mark.parametrize("layout", ["dense", "row"])
@pytest.mark.parametrize("index", ["none", "sorted", "unsorted"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D,Dy", SHAPES)
def test_adapted_draw_equals_contract(hip_device, B, K, D, Dy, dtype, index, layout):
    provider = _provider()
    gain, _, r, loc, eps = _operands(B, K, D, Dy, dtype, 11 * K + D)
    rng = np.random.RandomState(K)
    idx = None
    if index != "none":
        idx = rng.randint(0, K, size=(B, K))
        if index == "sorted":
            idx = np.sort(idx, axis=1)      # (with repeats: K draws from K values)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    device_loc, host_loc = _device_loc(loc, layout, hip_device)
    lower = gain["L"] + np.triu(np.full((D, D), np.nan), 1)      # nothing above the diagonal is read
    out = provider.adapted_draw(device_loc, dev(idx), dev(gain["M"]), dev(r), dev(lower), dev(eps))
    assert out.dtype == TORCH[dtype] and tuple(out.shape) == (B, K, D) and out.is_contiguous()
    want, flags = contract.adapted_draw(host_loc, idx, gain["M"], r, gain["L"], eps)
    bound = contract.adapted_draw_bound(host_loc, idx, gain["M"], r, gain["L"], eps)
    ok = _within(out.cpu().numpy(), want, bound, dtype)
    assert flags == 0 and ok.all(), (np.argwhere(~ok)[:4], np.abs(out.cpu().numpy() - want).max(), bound.max())
    assert provider.read_flags(hip_device) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_index_out_of_range_gives_nan_and_the_flag(hip_device, dtype):
    from aesmc_amd import _lib
    provider = _provider()
    B, K, D = 3, 300, 10
    gain, _, r, loc, eps = _operands(B, K, D, D, dtype, 5)
    idx = np.random.RandomState(0).randint(0, K, size=(B, K))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    clean = provider.adapted_draw(dev(loc), dev(idx), dev(gain["M"]), dev(r), dev(gain["L"]), dev(eps))
    assert provider.read_flags(hip_device) == 0
    bad = idx.copy()
    bad[0, 0], bad[1, 299], bad[2, 256] = K, -1, 1 << 40
    out = provider.adapted_draw(dev(loc), dev(bad), dev(gain["M"]), dev(r), dev(gain["L"]), dev(eps))
    assert provider.read_flags(hip_device) == _lib.FLAG_INDEX_OUT_OF_RANGE
    hit = torch.from_numpy(bad != idx).to(hip_device)
    assert torch.isnan(out[hit]).all() and torch.equal(out[~hit], clean[~hit])
    want, flags = contract.adapted_draw(loc, bad, gain["M"], r, gain["L"], eps)
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE and np.array_equal(np.isnan(want), np.isnan(out.cpu().numpy()))


def test_provider_refuses_what_the_kernels_do_not_take(hip_device):
    provider = _provider()
    loc = torch.zeros(2, 4, 3, device=hip_device)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=hip_device)
    assert provider.adapted_covers(loc, 3, 2) and not provider.adapted_covers(loc, 3, 17)
    assert not provider.adapted_covers(loc.cpu(), 3, 2) and not provider.adapted_covers(loc.half(), 3, 2)
    assert not provider.adapted_covers(torch.zeros(2, 4, 17, device=hip_device), 17, 2)
    with pytest.raises(ValueError, match="P must be"):
        provider.affine_quadratic_logweight(loc, f64(2, 4), f64(2, 2), 0.0)
    with pytest.raises(ValueError, match="offset must be"):
        provider.adapted_draw(loc, None, f64(3, 3), f64(2, 2), f64(3, 3), torch.zeros_like(loc))
    with pytest.raises(ValueError, match="noise must be"):
        provider.adapted_draw(loc, None, f64(3, 3), f64(2, 3), f64(3, 3), torch.zeros(2, 4, 3, dtype=torch.float64, device=hip_device))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        provider.affine_quadratic_logweight(loc.cpu(), f64(2, 3), f64(2, 2), 0.0)
    empty = provider.adapted_draw(loc[:0], None, f64(3, 3), f64(0, 3), f64(3, 3), torch.zeros_like(loc[:0]))
    assert tuple(empty.shape) == (0, 4, 3)


# ---- the whole filter -------------------------------------------------------------------------------------------------------
class _Feed:
    def __init__(self, blocks):
        self.blocks = list(blocks)

    def next(self):
        return self.blocks.pop(0)


def _model(family, dim, dtype, device):
    from aesmc_amd.testing.models import LgssmNd, NonlinearSsm
    if family == "lgssm":
        model = LgssmNd(dim, dtype=dtype, affine=True).to(device)
    else:
        model = NonlinearSsm(dim, dtype=dtype).to(device)
    A, C = model.A.detach().double().cpu().numpy(), model.C.detach().double().cpu().numpy()
    location = (lambda x, t: x @ A.T) if family == "lgssm" else (lambda x, t: np.tanh(x @ A.T))
    return model, A, C, location


@pytest.mark.parametrize("resampling", ["systematic", "stratified"])
@pytest.mark.parametrize("family", ["lgssm", "nonlinear"])
def test_whole_run_replayed_in_float64(hip_device, family, resampling):
    from aesmc_amd import adapted, inference
    T, B, K, d = 4, 4, 65, 3
    model, A, C, location = _model(family, d, torch.float64, hip_device)
    observations = model.simulate(T, B, seed=2)
    rng = np.random.RandomState(9)
    noise = [rng.randn(B, K, d) for _ in range(T)]
    uniforms = [rng.uniform(size=(B, K) if resampling == "stratified" else (B,)) for _ in range(T - 1)]
    want = contract.adapted_pass([y.cpu().numpy() for y in observations], np.zeros(d), np.ones(d), location, 1.0, C, None,
                                 0.5, noise, uniforms, lipschitz=float(np.abs(A).sum(axis=1).max()))
    assert want["flags"] == 0 and min(want["margins"]) > 1e-9, want["margins"]
    dev = lambda a: torch.from_numpy(a).to(hip_device)
    with inference.uniform_feed(_Feed(dev(u) for u in uniforms)):
        out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, K,
                                     resampling=resampling, noise=[dev(e) for e in noise], return_first_stage=True)
    for got, expected in zip(out["ancestral_indices"], want["ancestral_indices"]):
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), expected)
    for t, (got, expected) in enumerate(zip(out["original_latents"], want["latents"])):
        error = np.abs(got.cpu().numpy() - expected).max()
        assert error <= want["tolerances"]["latents"][t], (t, error, want["tolerances"]["latents"][t])
    for got, expected in zip(out["first_stage_log_weights"], want["first_stage_log_weights"]):
        assert np.abs(got.cpu().numpy() - expected).max() <= 1e-9
    error = np.abs(out["log_marginal_likelihood"].cpu().numpy() - want["log_marginal_likelihood"]).max()
    assert error <= want["tolerances"]["log_marginal_likelihood"], (error, want["tolerances"])
    assert want["tolerances"]["log_marginal_likelihood"] < 1e-9 and max(want["tolerances"]["latents"]) < 1e-9
    assert all(not w.any() and tuple(w.shape) == (B, K) for w in out["log_weights"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_step_is_the_exact_evidence(hip_device, dtype):
    from aesmc_amd import adapted
    from aesmc_amd.testing.models import kalman_log_likelihood
    model, A, C, _ = _model("lgssm", 3, dtype, hip_device)
    observations = model.simulate(1, 6, seed=4)
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, 33)
    got = out["log_marginal_likelihood"].cpu().numpy()
    if dtype == torch.float64:
        np.testing.assert_allclose(got, kalman_log_likelihood(model, observations), rtol=0, atol=1e-10)
    rng = np.random.RandomState(0)
    want = contract.adapted_pass([observations[0].double().cpu().numpy()], np.zeros(3), np.ones(3), None,
                                 float(model.transition_scale), C, None, float(model.emission_scale),
                                 [rng.randn(6, 33, 3)], [], dtype=np.float32 if dtype == torch.float32 else np.float64)
    assert np.abs(got - want["log_marginal_likelihood"]).max() <= want["tolerances"]["log_marginal_likelihood"]
    assert want["tolerances"]["log_marginal_likelihood"] < 1e-10
    assert tuple(out["last_latent"].shape) == (6, 33, 3) and out["last_latent"].dtype == dtype


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_unbiased_with_a_fraction_of_the_bootstrap_variance(hip_device, dtype):
    """The CPU test's setting (tests/test_adapted_contract.py: LgssmNd(2), T = 5, K = 64, 512 replicas of one observation
    sequence) on the device: exp(log Z-hat - exact) has mean 1 within 4 standard errors; log Z-hat's variance is below
    0.1 of `infer("smc")`'s with the transition as proposal (twice the CPU bound, for another random stream; the
    measured ratios are in profiles/adapted_filter.txt); the particle means of x_0 and of the last step lie within 5
    standard errors (over the replicas) of the Kalman filter's."""
    from aesmc_amd import adapted, inference
    T, K, R, d = 5, 64, 512, 2
    model, A, C, _ = _model("lgssm", d, dtype, hip_device)
    one = model.simulate(T, 1, seed=1)
    observations = [y.expand(R, d).contiguous() for y in one]
    torch.manual_seed(21)
    np.random.seed(21)
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, K)
    means, covs, exact = contract.kalman_filter(A, C, float(model.transition_scale), float(model.emission_scale), np.zeros(d),
                                                np.ones(d), [y.double().cpu().numpy() for y in one])
    log_z = out["log_marginal_likelihood"].double().cpu().numpy()
    ratio = np.exp(log_z - exact[0])
    z_score = abs(ratio.mean() - 1.0) / (ratio.std(ddof=1) / np.sqrt(R))

    def proposal(previous_latents=None, time=None, observations=None):
        if time == 0:
            return model.initial()
        return model.transition(previous_latents=previous_latents, time=time)

    with torch.no_grad():
        bootstrap = inference.infer("smc", observations, model.initial, model.transition, model.emission, proposal, K,
                                    return_log_marginal_likelihood=True, return_latents=False, return_log_weight=False)
    boot = bootstrap["log_marginal_likelihood"].detach().double().cpu().numpy()
    variance_ratio = log_z.var(ddof=1) / boot.var(ddof=1)
    print("adapted filter on the device, {}: z-score {:.3f}, var {:.3e}; bootstrap var {:.3e}; ratio {:.4f}".format(
        dtype, z_score, log_z.var(ddof=1), boot.var(ddof=1), variance_ratio))
    assert z_score <= 4.0
    assert variance_ratio < 0.1
    for t in (0, T - 1):
        per_replica = out["original_latents"][t].double().mean(dim=1).cpu().numpy()
        standard_error = per_replica.std(axis=0, ddof=1) / np.sqrt(R)
        z = np.abs(per_replica.mean(axis=0) - means[t, 0]) / standard_error
        print("  step {}: particle-mean z-scores {}".format(t, np.round(z, 3)))
        assert (z <= 5.0).all(), (t, z)


def test_nan_location_raises_at_the_end_and_the_next_call_starts_clean(hip_device):
    from aesmc_amd import adapted
    model, _, _, _ = _model("lgssm", 3, torch.float32, hip_device)
    observations = model.simulate(3, 2, seed=3)
    calls = []

    def poisoned(previous_latents=None, time=None, previous_observations=None):
        calls.append(time)
        loc = previous_latents[-1] @ model.A.t()
        loc[1, 5, 0] = float("nan")
        return model._tag(torch.distributions.Normal(loc, model.transition_scale, validate_args=False), "FULLY_EXPANDED")

    with pytest.raises(FloatingPointError):
        adapted.adapted_filter(observations, model.initial, poisoned, model.emission, 16)
    assert calls == [1, 2]      # raised at the end of the call, not at the step
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, 16)
    assert torch.isfinite(out["log_marginal_likelihood"]).all() and torch.isfinite(out["last_latent"]).all()


def test_the_output_feeds_the_smoothers_unchanged(hip_device):
    from aesmc_amd import adapted, smoothing
    T, B, K, d = 4, 3, 40, 3
    model, _, _, _ = _model("lgssm", d, torch.float32, hip_device)
    observations = model.simulate(T, B, seed=6)
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, K, return_latents=True)
    assert len(out["latents"]) == T and all(tuple(x.shape) == (B, K, d) for x in out["latents"])
    paths = smoothing.backward_simulate(out["original_latents"], out["log_weights"], model.transition, num_trajectories=7,
                                        observations=observations)
    assert len(paths) == T and all(tuple(x.shape) == (B, 7, d) and torch.isfinite(x).all() for x in paths)
    smoothed = smoothing.marginal_log_weights(out["original_latents"], out["log_weights"], model.transition,
                                              observations=observations)
    assert len(smoothed) == T and all(tuple(w.shape) == (B, K) and torch.isfinite(w).all() for w in smoothed)
    last = smoothed[-1].double()
    assert torch.allclose(last, torch.full_like(last, -np.log(K)), rtol=0, atol=1e-6)      # uniform at the last step
