"""Backward simulation (FFBS) on the device: kernel K21 (aesmc_backward_sample) against its NumPy contract
(aesmc_amd/testing/smoothing.py) — indices, flags and payload bits — its views, its conventions for bad rows, an
independent frequency check, and `aesmc_amd.smoothing` end to end: against the NumPy backward pass on the contract models
and against the exact (Rauch-Tung-Striebel) smoother on the suite's long random-walk problem."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract

pytestmark = pytest.mark.gpu

BELOW_ONE = 1.0 - 2.0 ** -53
SHAPES = [(1, 1, 1, 1), (2, 2, 3, 1), (3, 7, 5, 2), (2, 64, 64, 3), (2, 65, 33, 10), (3, 257, 100, 1), (2, 1000, 17, 10),
          (2, 1024, 256, 16), (2, 300, 40, 17), (1, 128, 16, 128), (1, 50, 4, 256), (1, 4097, 64, 10), (1, 33000, 8, 2),
          (3, 7, 5, 0), (2, 1024, 256, 0), (1, 33000, 8, 0)]
PROFILES = ("flat", "unit", "wide", "minus_inf_stretch", "tied", "dominant", "far")


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _operands(profile, B, K, M, D, dtype, seed):
    """(log_w, loc, target, scale, u, payload) as NumPy arrays of `dtype` (u float64) for one weight / score profile."""
    rng = np.random.RandomState(seed)
    log_w = rng.randn(B, K) * {"flat": 0.0, "wide": 10.0}.get(profile, 1.0)
    loc, target = rng.randn(B, K, D), rng.randn(B, M, D)
    scale = 0.5 + rng.rand(D)
    if profile == "minus_inf_stretch":
        log_w[:, K // 3:K // 3 + max(1, K // 4)] = -np.inf
        log_w[:, 0] = 0.0          # (K == 1: keep a particle)
    elif profile == "tied":        # every particle at the same location, equal weights: every score of a trajectory tied
        loc[:] = loc[:, :1]
        log_w[:] = 0.0
    elif profile == "dominant":
        log_w[np.arange(B), rng.randint(K, size=B)] += 60.0
    elif profile == "far":         # targets far from every location: most of w underflows to zero
        target += 400.0
    u = rng.rand(B, M)
    u[rng.randint(B, size=3), rng.randint(M, size=3)] = 0.0
    payload = rng.randn(B, K, 3)
    return (log_w.astype(dtype), loc.astype(dtype), target.astype(dtype), scale.astype(dtype), u, payload.astype(dtype))


def _launch(device, log_w, loc, target, scale, u, payload):
    """The kernel on NumPy operands -> (idx, flags, moved) as NumPy."""
    provider = _provider()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert provider.read_flags(device) == 0
    idx, moved = provider.backward_sample(dev(log_w), dev(loc), dev(target), dev(scale), dev(u), dev(payload))
    flags = provider.read_flags(device)
    return idx.cpu().numpy(), flags, None if moved is None else moved.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,M,D", SHAPES)
def test_kernel_equals_contract_exactly(hip_device, dtype, B, K, M, D):
    for number, profile in enumerate(PROFILES):
        if D == 0 and profile in ("tied", "far"):
            continue      # (no transition term: nothing to tie or to move away)
        log_w, loc, target, scale, u, payload = _operands(profile, B, K, M, max(D, 1), dtype, 100 * number + K % 89)
        if D == 0:
            loc = target = scale = None
        elif number % 2:
            scale = scale[:1]      # one value for the whole latent
        want_idx, want_flags, want_moved = contract.backward_sample(log_w, loc, target, scale, u, payload)
        idx, flags, moved = _launch(hip_device, log_w, loc, target, scale, u, payload)
        assert want_flags == 0 and flags == 0, (profile, flags)
        differ = np.argwhere(idx != want_idx)
        assert differ.size == 0, (profile, len(differ), differ[:4], idx[tuple(differ[0])], want_idx[tuple(differ[0])])
        assert moved.dtype == dtype and np.array_equal(moved.view(np.uint8), want_moved.view(np.uint8)), profile


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,M,D", [(2, 50, 9, 0), (2, 1000, 17, 3), (1, 4097, 16, 2)])
def test_the_clamp_lands_on_a_particle_of_positive_weight(hip_device, dtype, B, K, M, D):
    log_w, loc, target, scale, u, payload = _operands("unit", B, K, M, max(D, 1), dtype, K)
    log_w[:, K - K // 4:] = -np.inf          # a weightless tail ...
    log_w[0, K // 2:] = -3000.0              # ... and one whose weights underflow
    u[:] = BELOW_ONE
    if D == 0:
        loc = target = scale = None
    idx, flags, _ = _launch(hip_device, log_w, loc, target, scale, u, None)
    assert flags == 0 and (idx >= 0).all() and (idx < K).all()
    for b in range(B):
        w = contract.backward_weights(log_w[b], None if D == 0 else loc[b], np.zeros((M, 0)) if D == 0 else target[b],
                                      scale)[0]
        assert (w[np.arange(M), idx[b]] > 0).all(), (b, idx[b])


def test_views_give_what_dense_copies_give(hip_device):
    provider = _provider()
    B, K, M, D, P = 3, 300, 21, 5, 4
    gen = torch.Generator(device=hip_device).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=hip_device, generator=gen)
    log_w = rand(B, K)
    loc_kb = rand(K, B, D)                       # stored [K,B,D]
    target_big = rand(B, M + 7, D)
    payload_big = rand(B, K, 2 * P + 1)
    scale = 0.5 + torch.rand(D, device=hip_device, generator=gen)
    u = torch.rand(B, M, device=hip_device, dtype=torch.float64, generator=gen)
    loc, target, payload = loc_kb.transpose(0, 1), target_big[:, 3:3 + M], payload_big[:, :, 1::2]
    assert not loc.is_contiguous() and not target.is_contiguous() and not payload.is_contiguous()
    for s in (scale, scale[:1], scale[0]):
        dense = provider.backward_sample(log_w, loc.contiguous(), target.contiguous(), s.clone(), u, payload.contiguous())
        views = provider.backward_sample(log_w, loc, target, s, u, payload)
        assert torch.equal(dense[0], views[0]) and torch.equal(dense[1], views[1]) and views[1].shape == (B, M, P)
        want = contract.backward_sample(log_w.cpu().numpy(), loc.cpu().numpy(), target.cpu().numpy(),
                                        s.reshape(-1).cpu().numpy(), u.cpu().numpy(), payload.cpu().numpy())
        assert np.array_equal(views[0].cpu().numpy(), want[0]) and np.array_equal(views[1].cpu().numpy(), want[2])
    # a [B,K] latent is D = 1; a [B,K,2,3] one is D = 6 with the payload's trailing dims kept
    flat = provider.backward_sample(log_w, loc[..., 0], target[..., 0], scale[:1], u, loc[..., 0])
    assert flat[1].shape == (B, M) and torch.equal(flat[1], torch.gather(loc[..., 0], 1, flat[0]))
    loc6, target6 = rand(B, K, 2, 3), rand(B, M, 2, 3)
    six = provider.backward_sample(log_w, loc6, target6, scale[:1], u, loc6)
    same = provider.backward_sample(log_w, loc6.reshape(B, K, 6), target6.reshape(B, M, 6), scale[:1], u)
    assert six[1].shape == (B, M, 2, 3) and torch.equal(six[0], same[0])
    assert provider.read_flags(hip_device) == 0


def test_bad_rows_flag_and_leave_the_others_alone(hip_device):
    B, K, M, D = 4, 300, 21, 3
    log_w, loc, target, scale, u, payload = _operands("unit", B, K, M, D, np.float32, 5)
    clean, flags, _ = _launch(hip_device, log_w, loc, target, scale, u, payload)
    assert flags == 0
    everything = np.ones((B, M), dtype=bool)

    def check(bad_log_w, bad_loc, bad_target, affected, bit):
        want = contract.backward_sample(bad_log_w, bad_loc, bad_target, scale, u, payload)
        idx, flags, moved = _launch(hip_device, bad_log_w, bad_loc, bad_target, scale, u, payload)
        assert flags == bit == want[1]
        assert (idx[affected] == K).all() and (idx[~affected] == clean[~affected]).all() and (clean < K).all()
        assert np.array_equal(idx, want[0]) and np.array_equal(moved, want[2])      # (idx == K copies particle K - 1)
        assert _provider().read_flags(hip_device) == 0                              # the status word is clear afterwards

    row = lambda b: everything & (np.arange(B) == b)[:, None]
    nan_w = log_w.copy()
    nan_w[1, 70] = np.nan
    check(nan_w, loc, target, row(1), contract.FLAG_NAN_LOG_WEIGHT)
    nan_loc = loc.copy()
    nan_loc[2, 299, 1] = np.nan
    check(log_w, nan_loc, target, row(2), contract.FLAG_NAN_LOG_WEIGHT)
    nan_target = target.copy()
    nan_target[0, 13, 2] = np.nan          # one trajectory of one row
    one = np.zeros((B, M), dtype=bool)
    one[0, 13] = True
    check(log_w, loc, nan_target, one, contract.FLAG_NAN_LOG_WEIGHT)
    dead = log_w.copy()
    dead[3] = -np.inf
    check(dead, loc, target, row(3), contract.FLAG_DEGENERATE_ROW)
    hot = log_w.copy()
    hot[0, 0] = np.inf
    check(hot, loc, target, row(0), contract.FLAG_DEGENERATE_ROW)


def test_index_frequencies_are_the_categorical(hip_device):
    """Independent of the contract: with one target shared by all trajectories the counts are M * softmax(s) within
    5 sigma."""
    provider = _provider()
    B, K, M, D = 2, 16, 65536, 2
    gen = torch.Generator(device=hip_device).manual_seed(1)
    log_w = torch.randn(B, K, device=hip_device, generator=gen)
    loc = torch.randn(B, K, D, device=hip_device, generator=gen)
    point = torch.randn(B, 1, D, device=hip_device, generator=gen)
    scale = torch.tensor([0.8], device=hip_device)
    u = torch.rand(B, M, device=hip_device, dtype=torch.float64, generator=gen)
    idx, _ = provider.backward_sample(log_w, loc, point.expand(B, M, D), scale, u)
    assert provider.read_flags(hip_device) == 0
    s = log_w.double() - 0.5 * (((point.double() - loc.double()) / scale.double()) ** 2).sum(-1)
    p = torch.softmax(s, dim=1).cpu().numpy()
    for b in range(B):
        counts = np.bincount(idx[b].cpu().numpy(), minlength=K)
        assert counts.sum() == M and len(counts) == K
        sigma = np.sqrt(M * p[b] * (1 - p[b]))
        assert (np.abs(counts - M * p[b]) <= 5 * sigma + 1).all(), (counts, M * p[b])


# ---- through the API ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered(hip_device):
    """One SMC run on the contract LGSSM (d = 3, B = 4, K = 257, T = 6), shared and left unchanged."""
    from aesmc_amd import inference
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(3, affine=True).tune_proposal().to(hip_device)
    observations = model.simulate(6, 4, seed=1)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_latents=False, return_original_latents=True, return_log_weights=True)
    from aesmc_amd import _lazy
    # (plain tensors: the test's own callables below are handed these directly)
    return model, observations, [_lazy.real(x) for x in out["original_latents"]], out["log_weights"]


@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul", "tanh"])
def test_backward_simulate_equals_the_numpy_backward_pass(hip_device, filtered, form):
    from aesmc_amd import smoothing, state
    from aesmc_amd.linear_gaussian import AffineNormal
    model, observations, latents, log_weights = filtered
    full = state.BatchShapeMode.FULLY_EXPANDED
    offset = torch.linspace(-0.2, 0.2, 3, device=hip_device)
    scale = torch.tensor([0.9, 1.0, 1.2], device=hip_device)

    def location(x):
        if form == "tanh":
            return torch.tanh(x @ model.A.t())
        return x @ model.A.t() + offset

    def transition(previous_latents=None, time=None, previous_observations=None):
        assert len(previous_latents) == time and len(previous_observations) == time
        assert all(type(x) is torch.Tensor for x in previous_latents)
        if form == "affine_normal":
            return state.set_batch_shape_mode(AffineNormal(previous_latents[-1], model.A, scale, offset=offset), full)
        return state.set_batch_shape_mode(Normal(location(previous_latents[-1]), scale), full)

    T, (B, K, d), M = len(latents), latents[0].shape, 100
    gen = torch.Generator().manual_seed(3)
    uniforms = [torch.rand(B, M, dtype=torch.float64, generator=gen).to(hip_device) for _ in range(T)]
    got, indices = smoothing.backward_simulate(latents, log_weights, transition, num_trajectories=M,
                                               observations=observations, uniforms=uniforms, return_indices=True)
    # (the filter's outputs carry the model parameters' autograd history: the restatement reads their values)
    x = [latent.detach().cpu().numpy() for latent in latents]
    # the model's locations as the device forms them (K8's chain for the AffineNormal, the library's product else)
    with torch.no_grad():
        locations = [transition(previous_latents=[latent.detach() for latent in latents[:t + 1]], time=t + 1,
                                previous_observations=observations[:t + 1]).loc.cpu().numpy() for t in range(T - 1)]
    want, want_idx = contract.backward_pass(x, [w.detach().cpu().numpy() for w in log_weights], lambda t: locations[t],
                                            scale.cpu().numpy(), [u.cpu().numpy() for u in uniforms])
    for t in range(T):
        assert indices[t].dtype == torch.int64 and got[t].shape == (B, M, d) and not got[t].requires_grad
        assert np.array_equal(indices[t].cpu().numpy(), want_idx[t]), (form, t)
        assert torch.equal(got[t], torch.gather(latents[t], 1, indices[t].unsqueeze(-1).expand(B, M, d)))
        assert np.array_equal(got[t].cpu().numpy(), want[t])


def test_same_seed_same_trajectories_and_numpy_untouched(hip_device, filtered):
    from aesmc_amd import smoothing
    model, observations, latents, log_weights = filtered
    np.random.seed(4)
    before = np.random.get_state()
    torch.manual_seed(6)
    first = smoothing.backward_simulate(latents, log_weights, model.transition, observations=observations)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    assert first[0].shape == latents[0].shape          # M defaults to K
    torch.manual_seed(6)
    again = smoothing.backward_simulate(latents, log_weights, model.transition, observations=observations)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    other = smoothing.backward_simulate(latents, log_weights, model.transition, observations=observations)
    assert not all(torch.equal(a, b) for a, b in zip(first, other))


def test_smooth_is_infer_followed_by_backward_simulate(hip_device, filtered):
    from aesmc_amd import inference, smoothing
    model, observations, _, _ = filtered
    torch.manual_seed(2)
    np.random.seed(2)
    trajectories, log_z = smoothing.smooth(observations, model.initial, model.transition, model.emission, model.proposal,
                                           257, num_trajectories=64)
    assert len(trajectories) == 6 and trajectories[0].shape == (4, 64, 3) and log_z.shape == (4,)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want = smoothing.backward_simulate(out["original_latents"], out["log_weights"], model.transition, num_trajectories=64,
                                       observations=observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"])
    assert all(torch.equal(a, b) for a, b in zip(trajectories, want))


def test_smoothed_posterior_against_the_exact_smoother(hip_device):
    """The setting of test_gpu_reference_suite.py::test_smoothed_posterior_against_a_kalman_smoother (its data, parameters,
    B = 4, K = 1000, T = 100, its Rauch-Tung-Striebel recursion) with M = 1000 backward-simulated trajectories: RMSE of the
    trajectory means < 0.6, mean relative variance error < 0.15, at least 100 distinct values at t = 0 in every system,
    and all three strictly better than the genealogy (`infer`'s own `latents`) of the same run.  The bounds are from the
    NumPy contract alone on this problem (0.23-0.36, 0.048-0.066, 333-372 over three seeds x four systems) and lie below
    the best genealogy values (0.79, 0.21, 21): handing back the genealogy fails all three."""
    from aesmc_amd import inference, smoothing, state, statistics
    Modes = state.BatchShapeMode
    T, K, B, M = 100, 1000, 4, 1000
    rng = np.random.RandomState(0)
    grid = np.linspace(0, 3 * np.pi, T)
    y = 40 * (np.sin(grid) + 0.2 * rng.randn(T))
    m0, p0, q, r = 0.0, 100.0, 25.0, 64.0          # x_0 ~ N(m0, p0), x_t = x_{t-1} + N(0, q), y_t = x_t + N(0, r)
    filt_m, filt_p, pred_m, pred_p = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    mean, var = m0, p0
    for t in range(T):                               # scalar Kalman filter, keeping what the smoother needs
        if t > 0:
            var = var + q
        pred_m[t], pred_p[t] = mean, var
        gain = var / (var + r)
        mean, var = mean + gain * (y[t] - mean), (1 - gain) * var
        filt_m[t], filt_p[t] = mean, var
    smooth_m, smooth_p = filt_m.copy(), filt_p.copy()
    for t in range(T - 2, -1, -1):                   # Rauch-Tung-Striebel backward pass
        back = filt_p[t] / pred_p[t + 1]
        smooth_m[t] = filt_m[t] + back * (smooth_m[t + 1] - pred_m[t + 1])
        smooth_p[t] = filt_p[t] + back * back * (smooth_p[t + 1] - pred_p[t + 1])
    dev_t = lambda v: torch.tensor(v, device=hip_device, dtype=torch.float32)
    full = Modes.FULLY_EXPANDED

    def initial():
        return Normal(dev_t(m0), dev_t(np.sqrt(p0)))

    def transition(previous_latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(Normal(previous_latents[-1], dev_t(np.sqrt(q))), full)

    def emission(latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(Normal(latents[-1], dev_t(np.sqrt(r))), full)

    def proposal(previous_latents=None, time=None, observations=None):
        if time == 0:
            return state.set_batch_shape_mode(Normal(dev_t(m0), dev_t(np.sqrt(p0))), Modes.NOT_EXPANDED)
        return transition(previous_latents=previous_latents)

    observations = torch.from_numpy(y).float().to(hip_device).unsqueeze(-1).expand(T, B).contiguous()
    torch.manual_seed(1)
    np.random.seed(1)
    out = inference.infer("smc", observations, initial, transition, emission, proposal, K, return_original_latents=True,
                          return_log_weights=True)
    trajectories = smoothing.backward_simulate(out["original_latents"], out["log_weights"], transition,
                                               num_trajectories=M, observations=observations)
    assert len(trajectories) == T and trajectories[0].shape == (B, M)

    def figures(means, variances, first):
        rmse = np.sqrt(np.mean((means - smooth_m[:, None]) ** 2, axis=0))
        relative = np.mean(np.abs(variances - smooth_p[:, None]) / smooth_p[:, None], axis=0)
        distinct = np.array([len(np.unique(first[b])) for b in range(B)])
        return rmse, relative, distinct

    paths = torch.stack(trajectories).double().cpu().numpy()                      # [T, B, M], equally weighted
    ffbs = figures(paths.mean(axis=2), paths.var(axis=2), paths[0])
    weight = out["log_weight"]
    means = torch.stack([statistics.empirical_mean(latent, weight) for latent in out["latents"]]).double().cpu().numpy()
    variances = torch.stack([statistics.empirical_variance(latent, weight) for latent in out["latents"]])
    genealogy = figures(means, variances.double().cpu().numpy(), out["latents"][0].double().cpu().numpy())
    print("\n[backward simulation] rmse {} var rel err {} distinct at t=0 {}; genealogy: rmse {} var rel err {} distinct {}"
          .format(np.round(ffbs[0], 3), np.round(ffbs[1], 3), ffbs[2], np.round(genealogy[0], 3),
                  np.round(genealogy[1], 3), genealogy[2]))
    assert (ffbs[0] < 0.6).all(), ffbs[0]
    assert (ffbs[1] < 0.15).all(), ffbs[1]
    assert (ffbs[2] >= 100).all(), ffbs[2]
    assert (ffbs[0] < genealogy[0]).all() and (ffbs[1] < genealogy[1]).all() and (ffbs[2] > genealogy[2]).all()
