"""The two-slice particle smoother on the device: kernel K23 (aesmc_pairwise_mean) against its NumPy contract
(aesmc_amd/testing/smoothing.py) within the contract's own bound, its lane map exactly, every form of it, its views, its
conventions for special values, and `aesmc_amd.smoothing.two_slice_expectation` / `two_slice_smooth` end to end: against
the NumPy recursion on the contract models and against the exact (Rauch-Tung-Striebel) lag-one covariance on the suite's
long random-walk problem."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract
from tests.test_gpu_marginal_smoothing import PROFILES, _operands, filtered  # noqa: F401  (K22's operand profiles and fixture)

pytestmark = pytest.mark.gpu

# (B, R, C, D, P): below, at and off the tile of 16 row points, the 64 columns, the 16-wide payload quad; the limits of D and P
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 1, 2), (2, 15, 63, 3, 3), (2, 16, 64, 3, 16), (2, 17, 65, 10, 17), (3, 33, 257, 1, 10),
          (1, 9, 1000, 10, 33), (1, 5, 300, 17, 256), (1, 4, 50, 256, 4), (2, 5, 70, 0, 5), (1, 8, 4097, 2, 1)]
FORMS = (1, 2, 3)      # the matrix cores, the vector pipe 4 x 16 and 2 x 32


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _payload(B, C, P, dtype, seed):
    return (3 * np.random.RandomState(seed).randn(B, C, P)).astype(dtype)


def _launch(device, rows, cols, scale, col_a, payload, col_sub, row_add):
    """The kernel on NumPy operands -> (out, lse, flags) as NumPy."""
    provider = _provider()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert provider.read_flags(device) == 0
    out, lse = provider.pairwise_mean(dev(rows), dev(cols), dev(scale), dev(col_a), dev(payload), dev(col_sub), dev(row_add))
    flags = provider.read_flags(device)
    return out.cpu().numpy(), lse.cpu().numpy(), flags


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


def _case(profile, number, B, R, C, D, P, dtype):
    rows, cols, scale, col_a, col_sub, row_add = _operands(profile, B, R, C, max(D, 1), dtype, 100 * number + C % 89)
    if D == 0:
        rows, cols, scale = rows[:, :, :0], cols[:, :, :0], None
    elif number % 2:
        scale = scale[:1]      # one value for the whole point
    return rows, cols, scale, col_a, _payload(B, C, P, dtype, number + P), col_sub, row_add


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,R,C,D,P", SHAPES)
def test_kernel_equals_contract_within_its_bound(hip_device, dtype, B, R, C, D, P):
    for number, profile in enumerate(PROFILES):
        if D == 0 and profile in ("tied", "far"):
            continue      # (no distance term: nothing to tie or to move away)
        rows, cols, scale, col_a, payload, col_sub, row_add = _case(profile, number, B, R, C, D, P, dtype)
        # with and without col_sub / row_add: every profile with both and with one other combination
        for sub, add in {(True, True), (bool(number & 1), bool(number & 2))}:
            operands = (rows, cols, scale, col_a, payload, col_sub if sub else None, row_add if add else None)
            want, want_lse, want_flags = contract.pairwise_mean(*operands)
            out, lse, flags = _launch(hip_device, *operands)
            assert want_flags == 0 and flags == 0 and out.dtype == lse.dtype == dtype, (profile, flags)
            _held(out, want, contract.pairwise_mean_bound(*operands), (profile, sub, add))
            _held(lse, want_lse, contract.pairwise_lse_bound(*operands[:4], *operands[5:]), (profile, sub, add, "lse"))


@pytest.mark.parametrize("C", [64, 256])
def test_the_lane_map_is_exact(hip_device, C):
    """D = 0 and col_a = 0: every weight is 1, so out is the column mean of the payload — small integers that differ in
    every (c, p), whose sums are exact in float64 in any order.  A wrong row or column map of the matrix-core form, a wrong
    lane in the vector forms' merge or a rescale of the wrong accumulator cannot pass."""
    provider = _provider()
    B, R, P = 2, 16 + 1, 19
    index = torch.arange(C * P, dtype=torch.float64, device=hip_device).reshape(C, P)          # differs in every (c, p)
    payload = torch.stack([index - 1000.0 * b for b in range(B)])
    empty = torch.zeros(B, R, 0, dtype=torch.float64, device=hip_device)
    no_cols = torch.zeros(B, C, 0, dtype=torch.float64, device=hip_device)
    col_a = torch.zeros(B, C, dtype=torch.float64, device=hip_device)
    want = (payload.sum(dim=1) / C)[:, None, :].expand(B, R, P)
    try:
        for form in (0,) + FORMS:
            assert provider._lib.aesmc_test_set_pairwise_mean_form(form) == 0
            out, lse = provider.pairwise_mean(empty, no_cols, None, col_a, payload)
            assert torch.equal(out, want), form
            assert (lse - float(np.log(C))).abs().max() < 1e-14, form
            # a payload that is non-zero in one column only picks that column's weight out of every row point's sum
            one = torch.zeros_like(payload)
            one[:, C - 5, :] = payload[:, C - 5, :]
            out, _ = provider.pairwise_mean(empty, no_cols, None, col_a, one)
            assert torch.equal(out, (one.sum(dim=1) / C)[:, None, :].expand(B, R, P)), form
    finally:
        assert provider._lib.aesmc_test_set_pairwise_mean_form(0) == 0
    assert provider.read_flags(hip_device) == 0


def test_every_form_of_the_kernel_is_held_to_the_same_bound(hip_device):
    provider = _provider()
    shapes = (((2, 40, 300, 17, 5), "unit"), ((1, 19, 1100, 3, 40), "dominant"), ((2, 5, 70, 0, 16), "wide"),
              ((1, 33, 130, 2, 70), "minus_inf_stretch"))
    cases = [_case(profile, number, *shape, np.float64) for number, (shape, profile) in enumerate(shapes)]
    wants = [(contract.pairwise_mean(*ops), contract.pairwise_mean_bound(*ops),
              contract.pairwise_lse_bound(*ops[:4], *ops[5:])) for ops in cases]
    try:
        for form in FORMS:
            assert provider._lib.aesmc_test_set_pairwise_mean_form(form) == 0
            for ops, ((want, want_lse, _), bound, lse_bound) in zip(cases, wants):
                out, lse, flags = _launch(hip_device, *ops)
                assert flags == 0
                _held(out, want, bound, (form, out.shape))
                _held(lse, want_lse, lse_bound, (form, out.shape, "lse"))
        assert provider._lib.aesmc_test_set_pairwise_mean_form(4) == 1      # an unknown form is rejected
    finally:
        assert provider._lib.aesmc_test_set_pairwise_mean_form(0) == 0


def test_the_denominators_are_the_marginal_kernels_bit_for_bit(hip_device):
    """`lse` is what K22 writes for the same operands: the same scores, reference moves, sums and merge."""
    provider = _provider()
    for number, (B, R, C, D, P) in enumerate(((2, 17, 65, 10, 3), (1, 9, 1000, 3, 20))):
        ops = _case("unit", number, B, R, C, D, P, np.float32)
        dev = [None if a is None else torch.from_numpy(a).to(hip_device) for a in ops]
        _, lse = provider.pairwise_mean(*dev)
        assert torch.equal(lse, provider.pairwise_lse(*dev[:4], *dev[5:]))


def test_views_give_what_dense_copies_give(hip_device):
    provider = _provider()
    B, R, C, D = 3, 21, 300, 5
    gen = torch.Generator(device=hip_device).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=hip_device, generator=gen)
    col_a, col_sub, row_add = rand(B, C), rand(B, C), rand(B, R)
    cols_cb = rand(C, B, D)                      # stored [C,B,D]
    rows_big = rand(B, R + 7, 2 * D + 1)
    latents = rand(B, C, 2 * D)
    scale = 0.5 + torch.rand(D, device=hip_device, generator=gen)
    cols, rows, payload = cols_cb.transpose(0, 1), rows_big[:, 3:3 + R, 1::2], latents[:, :, ::2]
    assert not cols.is_contiguous() and not rows.is_contiguous() and not payload.is_contiguous()
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for s in (scale, scale[:1], scale[0]):
        dense = provider.pairwise_mean(rows.contiguous(), cols.contiguous(), s.clone(), col_a, payload.contiguous(), col_sub,
                                       row_add)
        views = provider.pairwise_mean(rows, cols, s, col_a, payload, col_sub, row_add)
        assert same(dense, views) and views[0].shape == (B, R, D) and views[1].shape == (B, R)
        assert views[0].dtype == views[1].dtype == col_a.dtype
        want, _, _ = contract.pairwise_mean(rows.cpu().numpy(), cols.cpu().numpy(), s.reshape(-1).cpu().numpy(),
                                            col_a.cpu().numpy(), payload.cpu().numpy(), col_sub.cpu().numpy(),
                                            row_add.cpu().numpy())
        assert np.abs(views[0].cpu().numpy() - want).max() < 1e-5
    # a payload that is the columns themselves, one that is a [B,C] tensor (P = 1), one of several trailing dims (P = 6)
    assert same(provider.pairwise_mean(rows, cols, scale, col_a, cols),
                provider.pairwise_mean(rows, cols, scale, col_a, cols.contiguous()))
    flat = provider.pairwise_mean(rows, cols, scale, col_a, latents[:, :, 3])
    assert flat[0].shape == (B, R, 1) and same(flat, provider.pairwise_mean(rows, cols, scale, col_a, latents[:, :, 3:4].contiguous()))
    six = rand(B, C, 2, 3)
    assert same(provider.pairwise_mean(rows, cols, scale, col_a, six),
                provider.pairwise_mean(rows, cols, scale, col_a, six.reshape(B, C, 6)))
    # an expanded point shared by all row points, and an expanded payload shared by all columns (it comes back as it is)
    point = rand(B, 1, D).expand(B, R, D)
    shared = provider.pairwise_mean(point, cols, scale, col_a, payload)
    assert same(shared, provider.pairwise_mean(point.contiguous(), cols, scale, col_a, payload))
    assert torch.equal(shared[0], shared[0][:, :1].expand(B, R, D))
    constant = rand(B, 1, 4).expand(B, C, 4)
    assert same(provider.pairwise_mean(rows, cols, scale, col_a, constant),
                provider.pairwise_mean(rows, cols, scale, col_a, constant.contiguous()))
    assert provider.read_flags(hip_device) == 0
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_mean(rows, cols, scale, col_a, payload.double())
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_mean(rows, cols, scale, col_a, payload[:, :-1])
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_mean(rows, cols, scale, col_a, rand(B, C, 257))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        provider.pairwise_mean(rows.cpu(), cols.cpu(), scale.cpu(), col_a.cpu(), payload.cpu())


def test_bad_row_points_flag_and_leave_the_others_alone(hip_device):
    B, R, C, D, P = 4, 21, 300, 3, 5
    rows, cols, scale, col_a, col_sub, row_add = _operands("unit", B, R, C, D, np.float32, 5)
    payload = _payload(B, C, P, np.float32, 6)
    clean, clean_lse, flags = _launch(hip_device, rows, cols, scale, col_a, payload, col_sub, row_add)
    assert flags == 0 and np.isfinite(clean).all()
    bits = lambda a: a.view(np.uint32)

    def check(affected, bit, value, lse_value, **changed):
        operands = dict(rows=rows, cols=cols, scale=scale, col_a=col_a, payload=payload, col_sub=col_sub, row_add=row_add)
        for name, (index, v) in changed.items():
            operands[name] = operands[name].copy()
            operands[name][index] = v
        want, want_lse, want_flags = contract.pairwise_mean(**operands)
        out, lse, flags = _launch(hip_device, **operands)
        assert flags == bit == want_flags, (changed, flags, want_flags)
        assert np.array_equal(out[affected], np.full((affected.sum(), P), value, dtype=np.float32), equal_nan=True), changed
        assert np.array_equal(lse[affected], np.full(affected.sum(), lse_value, dtype=np.float32), equal_nan=True), changed
        assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isnan(lse), np.isnan(want_lse))
        assert np.array_equal(bits(out[~affected]), bits(clean[~affected])), changed
        assert np.array_equal(bits(lse[~affected]), bits(clean_lse[~affected])), changed
        assert _provider().read_flags(hip_device) == 0          # the status word is clear afterwards

    everything = np.ones((B, R), dtype=bool)
    row = lambda b: everything & (np.arange(B) == b)[:, None]
    one = np.zeros((B, R), dtype=bool)
    one[0, 13] = True
    nan_flag, degenerate = contract.FLAG_NAN_LOG_WEIGHT, contract.FLAG_DEGENERATE_ROW
    check(row(1), nan_flag, np.nan, np.nan, col_a=((1, 70), np.nan))
    check(row(2), nan_flag, np.nan, np.nan, cols=((2, 299, 1), np.nan))
    check(row(2), nan_flag, np.nan, np.nan, col_sub=((2, 257), np.nan))
    check(one, nan_flag, np.nan, np.nan, rows=((0, 13, 2), np.nan))            # one row point of one batch row
    check(one, nan_flag, np.nan, np.nan, row_add=((0, 13), np.nan))
    check(everything, nan_flag, np.nan, np.nan, scale=(1, np.nan))
    check(row(3), degenerate, np.nan, np.inf, col_sub=((3, 5), -np.inf))
    check(row(0), degenerate, np.nan, np.inf, col_a=((0, 0), np.inf))
    check(row(3), 0, 0.0, -np.inf, col_a=((3, slice(None)), -np.inf))          # every column absent: zero weight, no flag
    check(one, 0, 0.0, -np.inf, rows=((0, 13, 0), np.inf))                     # infinitely far from every column
    # an absent column never reaches a result whatever its payload (and its col_sub) holds
    gone = [a.copy() for a in (rows, cols, scale, col_a, payload, col_sub, row_add)]
    gone[3][1, 40] = -np.inf
    reference = _launch(hip_device, *gone)
    assert reference[2] == 0 and np.isfinite(reference[0]).all()
    for held in (np.nan, np.inf, -np.inf):
        operands = [a.copy() for a in gone]
        operands[4][1, 40] = held
        operands[5][1, 40] = np.nan
        out, lse, flags = _launch(hip_device, *operands)
        assert flags == 0
        assert np.array_equal(bits(out), bits(reference[0])) and np.array_equal(bits(lse), bits(reference[1])), held
    assert np.array_equal(bits(np.delete(reference[0], 1, 0)), bits(np.delete(clean, 1, 0)))
    _held(reference[0], contract.pairwise_mean(*gone)[0], contract.pairwise_mean_bound(*gone), "absent")


# ---- through the API ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul", "tanh"])
def test_two_slice_expectation_equals_the_numpy_two_slice_pass(hip_device, filtered, form):  # noqa: F811
    from aesmc_amd import smoothing, state, statistics
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
    x = [latent.detach().cpu().numpy() for latent in latents]
    w = [weight.detach().cpu().numpy() for weight in log_weights]
    with torch.no_grad():
        locations = [transition(previous_latents=[latent.detach() for latent in latents[:t + 1]], time=t + 1,
                                previous_observations=observations[:t + 1]).loc.cpu().numpy() for t in range(T - 1)]
    marginal = smoothing.marginal_log_weights(latents, log_weights, transition, observations=observations)
    ones = lambda t, v: v.new_ones(v.shape[0], v.shape[1], 1)
    numpy_ones = lambda t, v: np.ones(v.shape[:2] + (1,), dtype=v.dtype)
    for previous, following, numpy_previous, numpy_following in ((None, None, None, None), (None, ones, None, numpy_ones),
                                                                 (ones, None, numpy_ones, None)):
        generator_before = torch.cuda.get_rng_state(hip_device)
        got, smoothed = smoothing.two_slice_expectation(latents, log_weights, transition, observations=observations,
                                                        previous=previous, following=following)
        assert torch.equal(generator_before, torch.cuda.get_rng_state(hip_device))      # no random stream consumed
        want, want_smoothed, (tolerance, smoothed_tolerance) = contract.two_slice_pass(
            x, w, lambda t: locations[t], scale.cpu().numpy(), numpy_previous, numpy_following, return_tolerance=True)
        assert len(got) == T - 1 and len(smoothed) == T
        for t in range(T):
            assert smoothed[t].shape == (B, K) and smoothed[t].dtype == log_weights[t].dtype
            error = np.abs(smoothed[t].cpu().numpy().astype(np.float64) - want_smoothed[t])
            assert (error <= smoothed_tolerance[t]).all(), (form, t, error.max())
            difference = np.abs((smoothed[t].double() - marginal[t].double()).cpu().numpy())
            assert (difference <= smoothed_tolerance[t]).all(), (form, t, difference.max())
        for t in range(T - 1):
            assert got[t].dtype == latents[0].dtype and not got[t].requires_grad
            mine = got[t].cpu().numpy().astype(np.float64)
            error = np.abs(mine - want[t])
            print("\n[two-slice smoother, {}] t = {}: largest difference {:.3e}, tolerance there {:.3e}".format(
                form, t, error.max(), tolerance[t].reshape(-1)[error.argmax()]))
            assert mine.shape == want[t].shape and (error <= tolerance[t]).all(), (form, t, error.max(), tolerance[t].min())
            # the marginalisation identities: following = 1 gives the means under smoothed[t], previous = 1 under smoothed[t+1]
            if previous is None and following is None:
                continue
            at = t if following is ones else t + 1
            weight = np.exp(smoothed[at].double().cpu().numpy())          # the device's weights, the mean in float64
            mean = np.einsum("bk,bkd->bd", weight, x[at].astype(np.float64))
            slack = np.einsum("bk,bkd->bd", weight * 2 * smoothed_tolerance[at], np.abs(x[at]).astype(np.float64))
            device_mean = statistics.empirical_mean(latents[at].detach(), smoothed[at]).double().cpu().numpy()
            assert np.abs(device_mean - mean).max() < 1e-4          # (`statistics` forms the same mean in float32)
            assert (np.abs(mine.reshape(B, d) - mean) <= tolerance[t].reshape(B, d) + slack).all(), (form, t)


def test_two_slice_smooth_is_infer_followed_by_two_slice_expectation(hip_device, filtered):  # noqa: F811
    from aesmc_amd import inference, smoothing
    model, observations, _, _ = filtered
    square = lambda t, v: torch.cat([v, v * v], dim=-1)
    torch.manual_seed(2)
    np.random.seed(2)
    latents, smoothed, expectations, log_z = smoothing.two_slice_smooth(
        observations, model.initial, model.transition, model.emission, model.proposal, 257, following=square)
    assert len(smoothed) == len(latents) == 6 and len(expectations) == 5 and expectations[0].shape == (4, 6, 3)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 257,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want, want_smoothed = smoothing.two_slice_expectation(out["original_latents"], out["log_weights"], model.transition,
                                                          observations=observations, following=square)
    assert torch.equal(log_z, out["log_marginal_likelihood"])
    assert all(torch.equal(a, b) for a, b in zip(expectations, want))
    assert all(torch.equal(a, b) for a, b in zip(smoothed, want_smoothed))
    with pytest.raises(NotImplementedError, match="P <= 256"):
        smoothing.two_slice_expectation(out["original_latents"], out["log_weights"], model.transition,
                                        observations=observations, previous=lambda t, v: v.new_zeros(4, 257, 257))
    assert _provider().read_flags(hip_device) == 0


def test_lag_one_covariance_against_the_exact_smoother(hip_device):
    """The setting of test_gpu_marginal_smoothing.py::test_smoothed_posterior_against_the_exact_smoother (its data,
    parameters, B = 4, K = 1000, T = 100, seed 1, its Rauch-Tung-Striebel recursion), extended by the exact lag-one
    covariance Cov(x_t, x_{t+1} | y) = back[t] * smooth_p[t+1].  The estimate is expectations[t] - mean_t * mean_{t+1};
    the metric the mean over t of |estimate - exact| / exact, per system: < 0.15 in every system and strictly smaller
    than the same metric of the genealogy of the same run.  The NumPy two-slice recursion behind a plain NumPy bootstrap
    filter on this problem (seeds 1-3, four systems each) gives 0.045-0.072 against the genealogy's 0.285-0.43, with
    exact lag-one covariances of 10.3-15.9.  This test's own run (seed 1) reads 0.063 0.077 0.051 0.055 against the
    genealogy's 0.391 0.360 0.389 0.329 on the device."""
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
    smooth_m, smooth_p, lag_one = filt_m.copy(), filt_p.copy(), np.zeros(T - 1)
    for t in range(T - 2, -1, -1):                   # Rauch-Tung-Striebel backward pass
        back = filt_p[t] / pred_p[t + 1]
        smooth_m[t] = filt_m[t] + back * (smooth_m[t + 1] - pred_m[t + 1])
        smooth_p[t] = filt_p[t] + back * back * (smooth_p[t + 1] - pred_p[t + 1])
        lag_one[t] = back * smooth_p[t + 1]          # Cov(x_t, x_{t+1} | y_0..y_{T-1})
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
    expectations, smoothed = smoothing.two_slice_expectation(stored, out["log_weights"], transition,
                                                             observations=observations)
    assert len(expectations) == T - 1 and expectations[0].shape == (B, 1, 1) and len(smoothed) == T

    def metric(cross, means):      # cross [T-1,B], means [T,B] -> [B]
        estimate = cross - means[:-1] * means[1:]
        return np.mean(np.abs(estimate - lag_one[:, None]) / lag_one[:, None], axis=0)

    means = torch.stack([statistics.empirical_mean(x, w) for x, w in zip(stored, smoothed)]).double().cpu().numpy()
    two_slice = metric(torch.stack([e.reshape(B) for e in expectations]).double().cpu().numpy(), means)
    paths = torch.stack([_lazy.real(x) for x in out["latents"]]).double()                                 # the genealogy: [T,B,K]
    weight = torch.softmax(out["log_weight"].double(), dim=1)                    # [B,K]
    genealogy = metric(((paths[:-1] * paths[1:]) * weight).sum(-1).cpu().numpy(), (paths * weight).sum(-1).cpu().numpy())
    print("\n[two-slice smoother] lag-one covariance, mean relative error {}; genealogy {}; exact {:.1f} .. {:.1f}".format(
        np.round(two_slice, 3), np.round(genealogy, 3), lag_one.min(), lag_one.max()))
    assert (two_slice < 0.15).all(), two_slice
    assert (two_slice < genealogy).all(), (two_slice, genealogy)
