"""The MAP trajectory (particle Viterbi) on the device: kernel K24 (aesmc_pairwise_argmax) against its NumPy contract
(aesmc_amd/testing/smoothing.py) within the contract's own bound and with the contract's own column, its tie rule across
lanes and chunks, its views, its conventions for special values, and `aesmc_amd.smoothing.map_trajectory` / `map_smooth`
end to end: against the NumPy recursion on the contract models, against the genealogy and backward simulation (K21), and
against the exact (Rauch-Tung-Striebel) smoother on the suite's long random-walk problem."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract
from tests.test_gpu_marginal_smoothing import PROFILES, _held, _operands

pytestmark = pytest.mark.gpu

# (B, R, C, D): R below, at and off the tile of 8 row points, more than one tile; C below, at and above a wavefront's 64
# columns (63, 64, 65), several chunks with a partial last one; D = 0, 1, the maximum, and no multiple of 4
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 1), (3, 5, 7, 2), (2, 9, 63, 3), (2, 8, 64, 3), (2, 17, 65, 10), (2, 33, 257, 1),
          (2, 17, 1000, 10), (2, 40, 300, 17), (1, 4, 50, 256), (3, 5, 7, 0), (1, 8, 1000, 0)]


def cases(shape, dtype):
    """(profile, tied, operands) of one shape: test_gpu_marginal_smoothing.py's profiles, each with col_sub and row_add
    and with one other combination of the two.  `tied`: the scores of a row point are equal by construction."""
    B, R, C, D = shape
    for number, profile in enumerate(PROFILES):
        if D == 0 and profile in ("tied", "far"):
            continue      # (no distance term: nothing to tie or to move away)
        rows, cols, scale, col_a, col_sub, row_add = _operands(profile, B, R, C, max(D, 1), dtype, 100 * number + C % 89)
        if D == 0:
            rows, cols, scale = rows[:, :, :0], cols[:, :, :0], None
        elif number % 2:
            scale = scale[:1]      # one value for the whole point
        for sub, add in sorted({(True, True), (bool(number & 1), bool(number & 2))}):
            tied = not sub and (profile == "tied" or (profile == "flat" and D == 0))
            yield profile, tied, (rows, cols, scale, col_a, col_sub if sub else None, row_add if add else None)


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _launch(device, rows, cols, scale, col_a, col_sub=None, row_add=None):
    """The kernel on NumPy operands -> (out, arg, flags) as NumPy."""
    provider = _provider()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert provider.read_flags(device) == 0
    out, arg = provider.pairwise_argmax(dev(rows), dev(cols), dev(scale), dev(col_a), dev(col_sub), dev(row_add))
    flags = provider.read_flags(device)
    assert arg.dtype == torch.int64 and arg.shape == out.shape
    return out.cpu().numpy(), arg.cpu().numpy(), flags


def _scores(rows, cols, scale, col_a, col_sub):
    """The contract's scores [B,R,C] in float64."""
    rows, cols, inv, col_a, col_sub, _ = contract._pairwise_operands(rows, cols, scale, col_a, col_sub, None)
    return np.stack([contract._pairwise_scores(rows[b], cols[b], inv, col_a[b], None if col_sub is None else col_sub[b])[0]
                     for b in range(rows.shape[0])])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,R,C,D", SHAPES)
def test_kernel_equals_contract_within_its_bound(hip_device, dtype, B, R, C, D):
    for profile, tied, operands in cases((B, R, C, D), dtype):
        want, want_arg, want_flags = contract.pairwise_argmax(*operands)
        bound = contract.pairwise_argmax_bound(*operands)
        gap = contract.pairwise_argmax_gap(*operands[:5])
        out, arg, flags = _launch(hip_device, *operands)
        what = (profile, operands[4] is not None, operands[5] is not None)
        assert want_flags == 0 and flags == 0 and out.dtype == dtype, (what, flags)
        _held(out, want, bound, what)
        assert ((arg >= 0) & (arg < C)).all(), what
        clear = gap > 2 * bound                      # the contract's winner is beyond any rounding: the same column
        assert np.array_equal(arg[clear], want_arg[clear]), what
        if tied:                                     # exact duplicates have identical bits: the smallest index, exactly
            assert np.array_equal(arg, want_arg), what
        else:                                        # elsewhere a column whose score is the maximum up to rounding ...
            assert 1000 * int((~clear).sum()) <= B * R, (what, int((~clear).sum()))      # ... for 1 row point in 1000
        if not clear.all():
            scores = _scores(*operands[:5])
            taken = np.take_along_axis(scores, arg[:, :, None], axis=2)[:, :, 0]
            assert (scores.max(axis=2) - taken <= 2 * bound)[~clear].all(), what


def test_ties_go_to_the_smallest_column_across_lanes_and_chunks(hip_device):
    """Exact duplicates of the best column in the same lane of a later chunk (c, c + 64), in neighbouring lanes (c, c + 1),
    and in a later chunk at a lower lane (5 and 66): the smaller index comes back, whichever of the two stood first."""
    B, R, C, D = 2, 11, 200, 3
    for dtype in (np.float32, np.float64):
        rows, cols, scale, col_a, col_sub, row_add = _operands("unit", B, R, C, D, dtype, 9)
        for first, second in ((7, 71), (70, 134), (30, 31), (63, 64), (5, 66), (66, 133), (0, 199)):
            c2, a2, s2 = cols.copy(), col_a.copy(), col_sub.copy()
            a2[:, first] = 80.0                       # the winner everywhere ...
            c2[:, second], a2[:, second], s2[:, second] = c2[:, first], a2[:, first], s2[:, first]      # ... and its twin
            out, arg, flags = _launch(hip_device, rows, c2, scale, a2, s2, row_add)
            assert flags == 0 and (arg == first).all(), (dtype, first, second, arg)
            alone = a2.copy()
            alone[:, second] = -np.inf                # without the twin: the same maximum, bit for bit
            assert np.array_equal(out, _launch(hip_device, rows, c2, scale, alone, s2, row_add)[0])
        # all columns identical with equal col_a: column 0, with and without a distance term
        same = np.ascontiguousarray(np.broadcast_to(cols[:, :1], cols.shape))
        for operands in ((rows, same, scale, np.zeros((B, C), dtype)), (rows[:, :, :0], cols[:, :, :0], None, np.full((B, C), 1.5, dtype))):
            out, arg, flags = _launch(hip_device, *operands)
            assert flags == 0 and (arg == 0).all()
            _held(out, contract.pairwise_argmax(*operands)[0], contract.pairwise_argmax_bound(*operands), "all tied")


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
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for s in (scale, scale[:1], scale[0]):
        dense = provider.pairwise_argmax(rows.contiguous(), cols.contiguous(), s.clone(), col_a, col_sub, row_add)
        views = provider.pairwise_argmax(rows, cols, s, col_a, col_sub, row_add)
        assert same(dense, views) and views[0].shape == views[1].shape == (B, R) and views[0].dtype == col_a.dtype
        want, want_arg, _ = contract.pairwise_argmax(rows.cpu().numpy(), cols.cpu().numpy(), s.reshape(-1).cpu().numpy(),
                                                     col_a.cpu().numpy(), col_sub.cpu().numpy(), row_add.cpu().numpy())
        assert np.abs(views[0].cpu().numpy() - want).max() < 1e-5 and np.array_equal(views[1].cpu().numpy(), want_arg)
    # the roles swapped, strided [B,*] operands, and an expanded point shared by all rows
    assert same(provider.pairwise_argmax(cols, rows, scale, row_add, None, col_a),
                provider.pairwise_argmax(cols.contiguous(), rows.contiguous(), scale, row_add, None, col_a))
    wide_a = rand(B, 2 * C)
    assert same(provider.pairwise_argmax(rows, cols, scale, wide_a[:, ::2]),
                provider.pairwise_argmax(rows, cols, scale, wide_a[:, ::2].contiguous()))
    point = rand(B, 1, D).expand(B, R, D)
    shared = provider.pairwise_argmax(point, cols, scale, col_a)
    assert same(shared, provider.pairwise_argmax(point.contiguous(), cols, scale, col_a))
    assert torch.equal(shared[0], shared[0][:, :1].expand(B, R)) and torch.equal(shared[1], shared[1][:, :1].expand(B, R))
    # a [B,R] tensor is D = 1; a [B,R,2,3] one is D = 6
    assert same(provider.pairwise_argmax(rows[..., 0], cols[..., 0], scale[:1], col_a),
                provider.pairwise_argmax(rows[..., :1], cols[..., :1], scale[:1], col_a))
    rows6, cols6 = rand(B, R, 2, 3), rand(B, C, 2, 3)
    assert same(provider.pairwise_argmax(rows6, cols6, scale[:1], col_a),
                provider.pairwise_argmax(rows6.reshape(B, R, 6), cols6.reshape(B, C, 6), scale[:1], col_a))
    assert provider.read_flags(hip_device) == 0
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_argmax(rows, cols, scale, col_a.double())
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_argmax(rows, cols[:, :-1], scale, col_a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        provider.pairwise_argmax(rows.cpu(), cols.cpu(), scale.cpu(), col_a.cpu())


def test_bad_row_points_flag_and_leave_the_others_alone(hip_device):
    B, R, C, D = 4, 21, 300, 3
    rows, cols, scale, col_a, col_sub, row_add = _operands("unit", B, R, C, D, np.float32, 5)
    clean, clean_arg, flags = _launch(hip_device, rows, cols, scale, col_a, col_sub, row_add)
    assert flags == 0 and np.isfinite(clean).all() and (clean_arg < C).all()

    def check(affected, bits, value, **changed):
        operands = dict(rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add)
        for name, edits in changed.items():
            operands[name] = operands[name].copy()
            for index, v in (edits if isinstance(edits, list) else [edits]):
                operands[name][index] = v
        want, want_arg, want_flags = contract.pairwise_argmax(**operands)
        out, arg, flags = _launch(hip_device, **operands)
        assert flags == bits == want_flags, (changed, flags, want_flags)
        if value is not None:
            assert np.array_equal(out[affected], np.full(affected.sum(), value, dtype=np.float32), equal_nan=True), changed
        assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isinf(out), np.isinf(want))
        assert np.array_equal(out[np.isinf(want)], want[np.isinf(want)].astype(np.float32))
        assert (arg[affected] == C).all() and np.array_equal(arg, want_arg), changed
        assert np.array_equal(out[~affected].view(np.uint32), clean[~affected].view(np.uint32)), changed
        assert np.array_equal(arg[~affected], clean_arg[~affected]), changed
        assert _provider().read_flags(hip_device) == 0          # the status word is clear afterwards

    everything = np.ones((B, R), dtype=bool)
    row = lambda b: everything & (np.arange(B) == b)[:, None]
    one = np.zeros((B, R), dtype=bool)
    one[0, 13] = True
    nan_flag, degenerate = contract.FLAG_NAN_LOG_WEIGHT, contract.FLAG_DEGENERATE_ROW
    check(row(1), nan_flag, np.nan, col_a=((1, 70), np.nan))
    check(row(2), nan_flag, np.nan, cols=((2, 299, 1), np.nan))          # (the last column: a partial chunk's last lane)
    check(row(2), nan_flag, np.nan, col_sub=((2, 257), np.nan))
    check(one, nan_flag, np.nan, rows=((0, 13, 2), np.nan))            # one row point of one batch row
    check(one, nan_flag, np.nan, row_add=((0, 13), np.nan))
    check(everything, nan_flag, np.nan, scale=(1, np.nan))
    check(row(3), degenerate, np.inf, col_sub=((3, 5), -np.inf))          # a present column over a col_sub of -inf
    check(row(0), degenerate, np.inf, col_a=((0, 0), np.inf))
    check(row(0), nan_flag, np.nan, col_a=[((0, 0), np.inf), ((0, 150), np.nan)])            # NaN wins over +inf
    check(row(0) | one, nan_flag | degenerate, None, col_a=((0, 0), np.inf), row_add=((0, 13), np.nan))
    check(row(1) | row(2), nan_flag | degenerate, None, col_a=[((1, 8), np.inf), ((2, 9), np.nan)])      # both flags
    check(row(3), 0, -np.inf, col_a=((3, slice(None)), -np.inf))          # every column absent: no column, no flag
    check(one, 0, -np.inf, rows=((0, 13, 0), np.inf))                     # infinitely far from every column
    # an absent column stays absent whatever col_sub holds: nothing is flagged, nothing is NaN, it is never the argument
    best = int(clean_arg[1, 0])
    for sub in (np.nan, -np.inf, np.inf):
        operands = [a.copy() for a in (rows, cols, scale, col_a, col_sub, row_add)]
        operands[3][1, best] = -np.inf
        operands[4][1, best] = sub
        out, arg, flags = _launch(hip_device, *operands)
        want, want_arg, _ = contract.pairwise_argmax(*operands)
        assert flags == 0 and np.isfinite(out).all() and arg[1, 0] != best and np.array_equal(arg, want_arg)
        _held(out, want, contract.pairwise_argmax_bound(*operands), sub)
        assert np.array_equal(np.delete(out, 1, 0), np.delete(clean, 1, 0))


# ---- through the API ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered(hip_device):
    """One SMC run on the contract LGSSM (d = 3, B = 4, K = 257, T = 6), shared and left unchanged: the setting of
    test_gpu_backward_simulation.py, with the genealogy kept too."""
    from aesmc_amd import _lazy, inference
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(3, affine=True).tune_proposal().to(hip_device)
    observations = model.simulate(6, 4, seed=1)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_latents=True, return_original_latents=True, return_log_weights=True)
    return model, observations, [_lazy.real(x) for x in out["original_latents"]], out["log_weights"], out["latents"]


def _log_normal(value, loc, scale):
    return (-0.5 * ((value - loc) / scale) ** 2 - np.log(scale) - 0.5 * np.log(2 * np.pi)).sum(-1)


@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul", "tanh"])
def test_map_trajectory_equals_the_numpy_viterbi_pass(hip_device, filtered, form):
    from aesmc_amd import smoothing, state
    from aesmc_amd.linear_gaussian import AffineNormal
    model, observations, latents, log_weights, genealogy = filtered
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
    trajectory, log_joint, indices = smoothing.map_trajectory(latents, model.initial, transition, model.emission,
                                                              observations, return_indices=True)
    assert torch.equal(generator_before, torch.cuda.get_rng_state(hip_device))      # deterministic: no stream consumed
    # the locations and the initial / emission log-densities as the device forms them
    detached = [latent.detach() for latent in latents]
    with torch.no_grad():
        locations = [transition(previous_latents=detached[:t + 1], time=t + 1,
                                previous_observations=observations[:t + 1]).loc.cpu().numpy() for t in range(T - 1)]
        initial_log_prob = state.log_prob(model.initial(), detached[0]).cpu().numpy()
        emission_log_probs = []
        for t in range(T):
            keywords = {} if t == 0 else dict(previous_observations=observations[:t])
            emission_log_probs.append(state.log_prob(model.emission(latents=detached[:t + 1], time=t, **keywords),
                                                     state.expand_observation(observations[t], K)).cpu().numpy())
    x = [latent.cpu().numpy() for latent in detached]
    want, want_joint, (tolerance, margin) = contract.viterbi_pass(x, initial_log_prob, emission_log_probs,
                                                                  lambda t: locations[t], scale.cpu().numpy(),
                                                                  return_tolerance=True)
    largest = max(t.max() for t in tolerance)
    print("\n[map trajectory, {}] smallest margin on the best paths {:.3e}, largest tolerance {:.3e}".format(
        form, margin.min(), largest))
    assert (margin > 2 * largest).all(), (form, margin, largest)          # asserted, not skipped: no rounding decides
    rows = torch.arange(B, device=hip_device)
    for t in range(T):
        assert indices[t].dtype == torch.int64 and np.array_equal(indices[t].cpu().numpy(), want[t]), (form, t)
        assert trajectory[t].shape == (B, d) and not trajectory[t].requires_grad
        assert torch.equal(trajectory[t], detached[t][rows, indices[t]])            # the stored values, bit for bit
    assert log_joint.shape == (B,) and log_joint.dtype == latents[0].dtype
    error = np.abs(log_joint.cpu().numpy().astype(np.float64) - want_joint)
    allowed = tolerance[-1].max(axis=1) + np.spacing(np.abs(want_joint).astype(np.float32)).astype(np.float64)
    assert (error <= allowed).all(), (form, error, allowed)
    if form != "affine_normal":
        return
    # the model's own joint density (NumPy, float64) of all 257 genealogy paths and of 257 backward-simulated trajectories
    # of the same run (under THIS transition): none beats the MAP path.  Slack: float32 densities, T (2 d + 1) terms of 1e-6
    A, C = model.A.detach().double().cpu().numpy(), model.C.detach().double().cpu().numpy()
    sy, y = float(model.emission_scale), [o.double().cpu().numpy() for o in observations]
    shift, sx = offset.double().cpu().numpy(), scale.double().cpu().numpy()
    torch.manual_seed(4)
    simulated = smoothing.backward_simulate(latents, log_weights, transition, num_trajectories=K, observations=observations)
    for name, paths in (("genealogy", genealogy), ("backward simulation", simulated)):
        paths = [p.detach().double().cpu().numpy() for p in paths]
        joint = _log_normal(paths[0], 0.0, np.ones(d))
        for t in range(T):
            joint = joint + _log_normal(y[t][:, None, :], paths[t] @ C.T, np.full(d, sy))
            if t > 0:
                joint = joint + _log_normal(paths[t], paths[t - 1] @ A.T + shift, sx)
        print("[map trajectory] log joint {} against the best of 257 {} paths {}".format(
            np.round(log_joint.cpu().numpy(), 3), name, np.round(joint.max(axis=1), 3)))
        assert (log_joint.double().cpu().numpy() >= joint.max(axis=1) - 1e-4).all(), (name, log_joint, joint.max(axis=1))


def test_map_smooth_is_infer_followed_by_map_trajectory(hip_device, filtered):
    from aesmc_amd import inference, smoothing
    model, observations = filtered[:2]
    torch.manual_seed(2)
    np.random.seed(2)
    trajectory, log_joint, log_z = smoothing.map_smooth(observations, model.initial, model.transition, model.emission,
                                                        model.proposal, 257)
    assert len(trajectory) == 6 and trajectory[0].shape == (4, 3) and log_joint.shape == (4,) and log_z.shape == (4,)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want, want_joint = smoothing.map_trajectory(out["original_latents"], model.initial, model.transition, model.emission,
                                                observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"]) and torch.equal(log_joint, want_joint)
    assert all(torch.equal(a, b) for a, b in zip(trajectory, want))


def test_map_trajectory_against_the_exact_smoother(hip_device):
    """The random-walk problem of test_gpu_marginal_smoothing.py::test_smoothed_posterior_against_the_exact_smoother (its
    data, parameters, B = 4, K = 1000, T = 100, seed 1, bootstrap proposal, its Rauch-Tung-Striebel recursion).  The RTS
    means are also the exact MAP path of this Gaussian model, and the joint density at them is the continuous maximum.
    Demanded of every system: RMSE of the MAP trajectory against the RTS means < 0.15 and strictly below that of the
    same run's FFBSm means; log_joint not above the closed-form joint at the RTS means (beyond rounding: 1e-3 on a
    float32 sum of 300 terms of size 5) and within 0.1 of it.  A NumPy bootstrap filter plus Viterbi on this problem gave
    RMSE 0.026-0.060 over six seeds (the cap leaves 2.5 x over the worst; the FFBSm means stand at 0.19-0.34, the filter
    means at 3.6-3.9) and a joint within 0.01 of the maximum.  This test's own run on the device (it prints them) reads
    RMSE 0.039 0.028 0.029 0.039 against the FFBSm means' 0.335 0.210 0.271 0.207, and log_joint -599.6357 -599.6344
    -599.6347 -599.6357 against the continuous maximum -599.6332: behind by 0.0024 0.0012 0.0015 0.0024."""
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
    smooth_m = filt_m.copy()
    for t in range(T - 2, -1, -1):                   # Rauch-Tung-Striebel backward pass (the means)
        smooth_m[t] = filt_m[t] + filt_p[t] / pred_p[t + 1] * (smooth_m[t + 1] - pred_m[t + 1])

    def joint_density(path):                         # log p(x_0..x_{T-1}, y_0..y_{T-1}) in float64, path [..., T]
        normal = lambda value, loc, variance: -0.5 * (value - loc) ** 2 / variance - 0.5 * np.log(2 * np.pi * variance)
        return (normal(path[..., 0], m0, p0) + normal(path[..., 1:], path[..., :-1], q).sum(-1) +
                normal(y, path, r).sum(-1))

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
    trajectory, log_joint = smoothing.map_trajectory(stored, initial, transition, emission, observations)
    assert len(trajectory) == T and trajectory[0].shape == (B,) and log_joint.shape == (B,)
    path = torch.stack(trajectory, dim=1).double().cpu().numpy()                                      # [B,T]
    smoothed = smoothing.marginal_log_weights(stored, out["log_weights"], transition, observations=observations)
    ffbsm = torch.stack([statistics.empirical_mean(x, w) for x, w in zip(stored, smoothed)], dim=1).double().cpu().numpy()
    rmse = np.sqrt(np.mean((path - smooth_m) ** 2, axis=1))
    rmse_ffbsm = np.sqrt(np.mean((ffbsm - smooth_m) ** 2, axis=1))
    top = joint_density(smooth_m)
    mine = log_joint.double().cpu().numpy()
    print("\n[map trajectory] rmse against the RTS means {} (FFBSm means: {}); log joint {} against the continuous "
          "maximum {:.4f}: behind by {}; the path's joint recomputed in float64 differs by {}".format(
              np.round(rmse, 4), np.round(rmse_ffbsm, 4), np.round(mine, 4), top, np.round(top - mine, 4),
              np.round(joint_density(path) - mine, 5)))
    assert (rmse < 0.15).all(), rmse
    assert (rmse < rmse_ffbsm).all(), (rmse, rmse_ffbsm)
    assert (mine <= top + 1e-3).all(), (mine, top)
    assert (mine >= top - 0.1).all(), (mine, top)
