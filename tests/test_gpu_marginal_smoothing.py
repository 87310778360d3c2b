"""The marginal particle smoother (FFBSm) on the device: kernel K22 (aesmc_pairwise_lse) against its NumPy contract
(aesmc_amd/testing/smoothing.py) within the contract's own bound, its views, its conventions for special values, and
`aesmc_amd.smoothing.marginal_log_weights` / `marginal_smooth` end to end: against the NumPy recursion on the contract
models, against backward simulation (K21) and against the exact (Rauch-Tung-Striebel) smoother on the suite's long
random-walk problem."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract

pytestmark = pytest.mark.gpu

# (B, R, C, D): R below, at and off the tile of 8 (16) row points; C below, at and above a wavefront's 64 columns and the
# 256 of the four-wavefront forms; D = 0, 1, the maximum, and no multiple of 4
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 1), (3, 5, 7, 2), (2, 64, 64, 3), (2, 33, 65, 10), (3, 100, 257, 1), (2, 17, 1000, 10),
          (2, 256, 1024, 16), (2, 40, 300, 17), (1, 16, 128, 128), (1, 4, 50, 256), (1, 64, 4097, 10), (1, 9, 33000, 2),
          (3, 5, 7, 0), (1, 8, 33000, 0)]
PROFILES = ("flat", "unit", "wide", "minus_inf_stretch", "tied", "dominant", "far")


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _operands(profile, B, R, C, D, dtype, seed):
    """(rows, cols, scale, col_a, col_sub, row_add) as NumPy arrays of `dtype` for one of K21's weight / score profiles
    (the columns are its particles, the row points its trajectories)."""
    rng = np.random.RandomState(seed)
    col_a = rng.randn(B, C) * {"flat": 0.0, "wide": 10.0}.get(profile, 1.0)
    cols, rows = rng.randn(B, C, D), rng.randn(B, R, D)
    scale = 0.5 + rng.rand(D)
    if profile == "minus_inf_stretch":
        col_a[:, C // 3:C // 3 + max(1, C // 4)] = -np.inf
        col_a[:, 0] = 0.0          # (C == 1: keep a column)
    elif profile == "tied":        # every column at the same place, equal weights: every score of a row point tied
        cols[:] = cols[:, :1]
        col_a[:] = 0.0
    elif profile == "dominant":    # the maximum sits late in the row: the reference has to move when it comes
        col_a[np.arange(B), rng.randint(C - 1 - C // 4, C, size=B)] += 60.0
    elif profile == "far":         # row points far from every column: the scores are large, most of the sum underflows
        rows += 400.0
    col_sub, row_add = rng.randn(B, C), rng.randn(B, R)
    return tuple(a.astype(dtype) for a in (rows, cols, scale, col_a, col_sub, row_add))


def _launch(device, rows, cols, scale, col_a, col_sub, row_add):
    """The kernel on NumPy operands -> (out, flags) as NumPy."""
    provider = _provider()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert provider.read_flags(device) == 0
    out = provider.pairwise_lse(dev(rows), dev(cols), dev(scale), dev(col_a), dev(col_sub), dev(row_add))
    flags = provider.read_flags(device)
    return out.cpu().numpy(), flags


def _held(out, want, bound, what):
    """float64: within the bound of the contract's value; float32: the float32 rounding of the contract's value, or its
    neighbour within the bound plus one float32 unit in the last place."""
    assert out.shape == want.shape and np.isfinite(want).all() and np.isfinite(out).all(), what
    error = np.abs(out.astype(np.float64) - want)
    if out.dtype == np.float64:
        allowed = bound
    else:
        allowed = np.where(out == want.astype(np.float32), np.inf, bound + np.spacing(np.abs(want).astype(np.float32)))
    worst = np.unravel_index(np.argmax(error - allowed), error.shape)
    assert (error <= allowed).all(), (what, worst, out[worst], want[worst], error[worst], bound[worst])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,R,C,D", SHAPES)
def test_kernel_equals_contract_within_its_bound(hip_device, dtype, B, R, C, D):
    for number, profile in enumerate(PROFILES):
        if D == 0 and profile in ("tied", "far"):
            continue      # (no distance term: nothing to tie or to move away)
        rows, cols, scale, col_a, col_sub, row_add = _operands(profile, B, R, C, max(D, 1), dtype, 100 * number + C % 89)
        if D == 0:
            rows, cols, scale = rows[:, :, :0], cols[:, :, :0], None
        elif number % 2:
            scale = scale[:1]      # one value for the whole point
        # with and without col_sub / row_add: every profile with both and with one other combination
        for sub, add in {(True, True), (bool(number & 1), bool(number & 2))}:
            operands = (rows, cols, scale, col_a, col_sub if sub else None, row_add if add else None)
            want, want_flags = contract.pairwise_lse(*operands)
            out, flags = _launch(hip_device, *operands)
            assert want_flags == 0 and flags == 0 and out.dtype == dtype, (profile, flags)
            _held(out, want, contract.pairwise_lse_bound(*operands), (profile, sub, add))


def test_every_form_of_the_kernel_is_held_to_the_same_bound(hip_device):
    """The tile heights, workgroup sizes and the two-pass form that tools/pairwise_lse_bench.py measures beside the
    default."""
    provider = _provider()
    cases = [(shape, _operands(profile, *shape, np.float64, 7)) for shape, profile in
             (((2, 40, 300, 17), "unit"), ((1, 19, 1100, 3), "dominant"), ((2, 5, 70, 0), "wide"))]
    cases = [(shape, ops if shape[3] else (ops[0][:, :, :0], ops[1][:, :, :0], None) + ops[3:]) for shape, ops in cases]
    wants = [(contract.pairwise_lse(*ops)[0], contract.pairwise_lse_bound(*ops)) for _, ops in cases]
    try:
        for tile in (8, 16):
            for waves in (1, 4):
                for passes in (1, 2):
                    assert provider._lib.aesmc_test_set_pairwise_lse_form(tile, waves, passes) == 0
                    for (shape, ops), (want, bound) in zip(cases, wants):
                        out, flags = _launch(hip_device, *ops)
                        assert flags == 0
                        _held(out, want, bound, (tile, waves, passes, shape))
        assert provider._lib.aesmc_test_set_pairwise_lse_form(12, 4, 1) == 1
    finally:
        assert provider._lib.aesmc_test_set_pairwise_lse_form(0, 0, 0) == 0


def test_views_give_what_dense_copies_give(hip_device):
    provider = _provider()
    B, R, C, D = 3, 21, 300, 5
    gen = torch.Generator(device=hip_device).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=hip_device, generator=gen)
    col_a, col_sub, row_add = rand(B, C), rand(B, C), rand(B, R)
    cols_cb = rand(C, B, D)                      # stored [C,B,D]
    rows_big = rand(B, R + 7, 2 * D + 1)
    scale = 0.5 + torch.rand(D, device=hip_device, generator=gen)
    cols, rows = cols_cb.transpose(0, 1), rows_big[:, 3:3 + R, 1::2]
    assert not cols.is_contiguous() and not rows.is_contiguous()
    for s in (scale, scale[:1], scale[0]):
        dense = provider.pairwise_lse(rows.contiguous(), cols.contiguous(), s.clone(), col_a, col_sub, row_add)
        views = provider.pairwise_lse(rows, cols, s, col_a, col_sub, row_add)
        assert torch.equal(dense, views) and views.shape == (B, R) and views.dtype == col_a.dtype
        want, _ = contract.pairwise_lse(rows.cpu().numpy(), cols.cpu().numpy(), s.reshape(-1).cpu().numpy(),
                                        col_a.cpu().numpy(), col_sub.cpu().numpy(), row_add.cpu().numpy())
        assert np.abs(views.cpu().numpy() - want).max() < 1e-5
    # the roles swapped (the smoother's second launch), strided [B,*] operands, and an expanded point shared by all rows
    swapped = provider.pairwise_lse(cols, rows, scale, row_add, None, col_a)
    assert torch.equal(swapped, provider.pairwise_lse(cols.contiguous(), rows.contiguous(), scale, row_add, None, col_a))
    wide_a = rand(B, 2 * C)
    assert torch.equal(provider.pairwise_lse(rows, cols, scale, wide_a[:, ::2]),
                       provider.pairwise_lse(rows, cols, scale, wide_a[:, ::2].contiguous()))
    point = rand(B, 1, D).expand(B, R, D)
    shared = provider.pairwise_lse(point, cols, scale, col_a)
    assert torch.equal(shared, provider.pairwise_lse(point.contiguous(), cols, scale, col_a))
    assert torch.equal(shared, shared[:, :1].expand(B, R))
    # a [B,R] tensor is D = 1; a [B,R,2,3] one is D = 6
    flat = provider.pairwise_lse(rows[..., 0], cols[..., 0], scale[:1], col_a)
    assert torch.equal(flat, provider.pairwise_lse(rows[..., :1], cols[..., :1], scale[:1], col_a))
    rows6, cols6 = rand(B, R, 2, 3), rand(B, C, 2, 3)
    assert torch.equal(provider.pairwise_lse(rows6, cols6, scale[:1], col_a),
                       provider.pairwise_lse(rows6.reshape(B, R, 6), cols6.reshape(B, C, 6), scale[:1], col_a))
    assert provider.read_flags(hip_device) == 0
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_lse(rows, cols, scale, col_a.double())
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_lse(rows, cols[:, :-1], scale, col_a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        provider.pairwise_lse(rows.cpu(), cols.cpu(), scale.cpu(), col_a.cpu())


def test_bad_row_points_flag_and_leave_the_others_alone(hip_device):
    B, R, C, D = 4, 21, 300, 3
    rows, cols, scale, col_a, col_sub, row_add = _operands("unit", B, R, C, D, np.float32, 5)
    clean, flags = _launch(hip_device, rows, cols, scale, col_a, col_sub, row_add)
    assert flags == 0 and np.isfinite(clean).all()

    def check(affected, bit, value, **changed):
        operands = dict(rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add)
        for name, (index, v) in changed.items():
            operands[name] = operands[name].copy()
            operands[name][index] = v
        want, want_flags = contract.pairwise_lse(**operands)
        out, flags = _launch(hip_device, **operands)
        assert flags == bit == want_flags, (changed, flags, want_flags)
        assert np.array_equal(out[affected], np.full(affected.sum(), value, dtype=np.float32), equal_nan=True), changed
        assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isinf(out), np.isinf(want))
        assert np.array_equal(out[~affected].view(np.uint32), clean[~affected].view(np.uint32)), changed
        assert _provider().read_flags(hip_device) == 0          # the status word is clear afterwards

    everything = np.ones((B, R), dtype=bool)
    row = lambda b: everything & (np.arange(B) == b)[:, None]
    one = np.zeros((B, R), dtype=bool)
    one[0, 13] = True
    nan_flag, degenerate = contract.FLAG_NAN_LOG_WEIGHT, contract.FLAG_DEGENERATE_ROW
    check(row(1), nan_flag, np.nan, col_a=((1, 70), np.nan))
    check(row(2), nan_flag, np.nan, cols=((2, 299, 1), np.nan))
    check(row(2), nan_flag, np.nan, col_sub=((2, 257), np.nan))
    check(one, nan_flag, np.nan, rows=((0, 13, 2), np.nan))            # one row point of one batch row
    check(one, nan_flag, np.nan, row_add=((0, 13), np.nan))
    check(everything, nan_flag, np.nan, scale=(1, np.nan))
    check(row(3), degenerate, np.inf, col_sub=((3, 5), -np.inf))          # a present column over a denominator without mass
    check(row(0), degenerate, np.inf, col_a=((0, 0), np.inf))
    check(row(3), 0, -np.inf, col_a=((3, slice(None)), -np.inf))          # every column absent: zero weight, no flag
    check(one, 0, -np.inf, rows=((0, 13, 0), np.inf))                     # infinitely far from every column
    # an absent column stays absent whatever col_sub holds: nothing is flagged, nothing is NaN
    for sub in (np.nan, -np.inf, np.inf):
        operands = [a.copy() for a in (rows, cols, scale, col_a, col_sub, row_add)]
        operands[3][1, 40] = -np.inf
        operands[4][1, 40] = sub
        out, flags = _launch(hip_device, *operands)
        want, _ = contract.pairwise_lse(*operands)
        assert flags == 0 and np.isfinite(out).all()
        _held(out, want, contract.pairwise_lse_bound(*operands), sub)
        assert np.array_equal(np.delete(out, 1, 0), np.delete(clean, 1, 0))


# ---- through the API ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered(hip_device):
    """One SMC run on the contract LGSSM (d = 3, B = 4, K = 257, T = 6), shared and left unchanged: the setting of
    test_gpu_backward_simulation.py."""
    from aesmc_amd import _lazy, inference
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(3, affine=True).tune_proposal().to(hip_device)
    observations = model.simulate(6, 4, seed=1)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_latents=False, return_original_latents=True, return_log_weights=True)
    return model, observations, [_lazy.real(x) for x in out["original_latents"]], out["log_weights"]


@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul", "tanh"])
def test_marginal_log_weights_equals_the_numpy_marginal_pass(hip_device, filtered, form):
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

    T, (B, K, d) = len(latents), latents[0].shape
    generator_before = torch.cuda.get_rng_state(hip_device)
    got = smoothing.marginal_log_weights(latents, log_weights, transition, observations=observations)
    assert torch.equal(generator_before, torch.cuda.get_rng_state(hip_device))      # deterministic: no stream consumed
    x = [latent.detach().cpu().numpy() for latent in latents]
    # the model's locations as the device forms them (K8's chain for the AffineNormal, the library's product else)
    with torch.no_grad():
        locations = [transition(previous_latents=[latent.detach() for latent in latents[:t + 1]], time=t + 1,
                                previous_observations=observations[:t + 1]).loc.cpu().numpy() for t in range(T - 1)]
    want, tolerance = contract.marginal_pass(x, [w.detach().cpu().numpy() for w in log_weights], lambda t: locations[t],
                                             scale.cpu().numpy(), return_tolerance=True)
    for t in range(T):
        assert got[t].shape == (B, K) and got[t].dtype == log_weights[t].dtype and not got[t].requires_grad
        mine = got[t].cpu().numpy().astype(np.float64)
        error = np.abs(mine - want[t].astype(np.float64))
        print("\n[marginal smoother, {}] t = {}: largest difference {:.3e}, tolerance there {:.3e}".format(
            form, t, error.max(), tolerance[t].reshape(-1)[error.argmax()]))
        assert (error <= tolerance[t]).all(), (form, t, error.max(), tolerance[t].min())
        top = mine.max(axis=1)
        total = top + np.log(np.exp(mine - top[:, None]).sum(axis=1))
        assert (np.abs(total) <= tolerance[t].max(axis=1)).all(), (form, t, total)      # rows sum to one
    assert (np.abs(got[0].cpu().numpy() - (log_weights[0] - torch.logsumexp(log_weights[0], 1, keepdim=True))
                   .detach().cpu().numpy()).max() > 1e-3)                                 # ... and are not the filter's


def test_marginal_smooth_is_infer_followed_by_marginal_log_weights(hip_device, filtered):
    from aesmc_amd import inference, smoothing
    model, observations, _, _ = filtered
    torch.manual_seed(2)
    np.random.seed(2)
    latents, smoothed, log_z = smoothing.marginal_smooth(observations, model.initial, model.transition, model.emission,
                                                         model.proposal, 257)
    assert len(smoothed) == len(latents) == 6 and smoothed[0].shape == (4, 257) and log_z.shape == (4,)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want = smoothing.marginal_log_weights(out["original_latents"], out["log_weights"], model.transition,
                                          observations=observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"])
    assert all(torch.equal(a, b) for a, b in zip(smoothed, want))
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(latents, out["original_latents"]))


def test_backward_simulation_frequencies_are_the_marginal_weights(hip_device):
    """K21 against K22: over M = 20 000 backward-simulated trajectories the number that pass through stored particle k at
    step t lies within 5 sigma + 1 of M exp(marginal log-weight) (B = 2, K = 64, T = 4);
    test_marginal_smoothing_contract.py shows that the two contracts alone stay inside that."""
    from aesmc_amd import _lazy, inference, smoothing
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(2, affine=True).tune_proposal().to(hip_device)
    T, B, K, M = 4, 2, 64, 20000
    observations = model.simulate(T, B, seed=3)
    torch.manual_seed(5)
    np.random.seed(5)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                          return_latents=False, return_original_latents=True, return_log_weights=True)
    latents, log_weights = [_lazy.real(x) for x in out["original_latents"]], out["log_weights"]
    smoothed = smoothing.marginal_log_weights(latents, log_weights, model.transition, observations=observations)
    _, indices = smoothing.backward_simulate(latents, log_weights, model.transition, num_trajectories=M,
                                             observations=observations, return_indices=True)
    for t in range(T):
        p = torch.exp(smoothed[t].double()).cpu().numpy()
        for b in range(B):
            counts = np.bincount(indices[t][b].cpu().numpy(), minlength=K)
            sigma = np.sqrt(M * p[b] * (1 - p[b]))
            assert counts.sum() == M and (np.abs(counts - M * p[b]) <= 5 * sigma + 1).all(), (t, b, counts, M * p[b])


def test_smoothed_posterior_against_the_exact_smoother(hip_device):
    """The setting of test_gpu_backward_simulation.py::test_smoothed_posterior_against_the_exact_smoother (its data,
    parameters, B = 4, K = 1000, T = 100, its Rauch-Tung-Striebel recursion) with the marginal smoother's weights on the
    stored particles, read through `statistics.empirical_mean / empirical_variance / ess`: RMSE of the smoothed means
    < 0.6, mean relative variance error < 0.15, an effective sample size at t = 0 of at least 100 in every system, and
    all three strictly better than the genealogy (`infer`'s own `latents`; its distinct values at t = 0 for the third)
    of the same run.  The caps are the backward-simulation test's.  The NumPy recursion behind a plain bootstrap filter
    on this problem gives 0.20-0.33, 0.038-0.061 and 287-334 over three seeds x four systems, against the genealogy's
    0.87-1.48, 0.21-0.31 and 10-18: handing back the filter weights or the genealogy fails all three.  The same recursion
    in NumPy (the contract's `marginal_pass`) on the DEVICE filter's stored particles, seeds 1-3 x four systems, gives
    0.19-0.34, 0.040-0.054 and 292-333 against the genealogy's 0.89-1.32, 0.21-0.26 and 12-18; this test's own run (seed
    1) reads 0.335 0.210 0.271 0.207, 0.046 0.054 0.040 0.042 and 306 309 302 333 on the device."""
    from aesmc_amd import _lazy, inference, smoothing, state, statistics
    Modes = state.BatchShapeMode
    T, K, B = 100, 1000, 4
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
    stored = [_lazy.real(x) for x in out["original_latents"]]
    smoothed = smoothing.marginal_log_weights(stored, out["log_weights"], transition, observations=observations)
    assert len(smoothed) == T and smoothed[0].shape == (B, K)

    def figures(latents, weights, spread):
        means = torch.stack([statistics.empirical_mean(x, w) for x, w in zip(latents, weights)]).double().cpu().numpy()
        variances = torch.stack([statistics.empirical_variance(x, w) for x, w in zip(latents, weights)]).double().cpu().numpy()
        rmse = np.sqrt(np.mean((means - smooth_m[:, None]) ** 2, axis=0))
        relative = np.mean(np.abs(variances - smooth_p[:, None]) / smooth_p[:, None], axis=0)
        return rmse, relative, spread

    ffbsm = figures(stored, smoothed, statistics.ess(smoothed[0]).double().cpu().numpy())
    first = out["latents"][0].double().cpu().numpy()
    genealogy = figures(out["latents"], [out["log_weight"]] * T, np.array([len(np.unique(first[b])) for b in range(B)]))
    print("\n[marginal smoother] rmse {} var rel err {} ess at t=0 {}; genealogy: rmse {} var rel err {} distinct {}"
          .format(np.round(ffbsm[0], 3), np.round(ffbsm[1], 3), np.round(ffbsm[2], 1), np.round(genealogy[0], 3),
                  np.round(genealogy[1], 3), genealogy[2]))
    assert (ffbsm[0] < 0.6).all(), ffbsm[0]
    assert (ffbsm[1] < 0.15).all(), ffbsm[1]
    assert (ffbsm[2] >= 100).all(), ffbsm[2]
    assert (ffbsm[0] < genealogy[0]).all() and (ffbsm[1] < genealogy[1]).all() and (ffbsm[2] > genealogy[2]).all()
