"""CPU checks of the marginal particle smoother (FFBSm): the NumPy contract of aesmc_pairwise_lse
(aesmc_amd/testing/smoothing.py) against a loop over every (row point, column) pair, its conventions for special values,
the backward recursion against explicit [K,K] matrices, the ABI's argument checks, the host logic of
`aesmc_amd.smoothing.marginal_log_weights` / `marginal_smooth` on a provider that adds `pairwise_lse` from the contract to
the suite's oracle provider, and the two smoothers' contracts against each other."""
import math

import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract
from tests.oracle_provider import OracleKernels


def _operands(rng, B, R, C, D, dtype=np.float64, vector_scale=True):
    rows, cols = rng.randn(B, R, D).astype(dtype), rng.randn(B, C, D).astype(dtype)
    scale = (0.5 + rng.rand(D if vector_scale else 1)).astype(dtype)
    col_a, col_sub, row_add = (2 * rng.randn(B, C)).astype(dtype), rng.randn(B, C).astype(dtype), rng.randn(B, R).astype(dtype)
    return rows, cols, scale, col_a, col_sub, row_add


def brute_force(rows, cols, scale, col_a, col_sub, row_add):
    """One pair at a time in Python floats (IEEE float64): a true division by the scale, math.exp, exact sums (fsum)."""
    B, R, D = rows.shape
    C = cols.shape[1]
    out = np.empty((B, R))
    for b in range(B):
        for r in range(R):
            s = []
            for c in range(C):
                q = math.fsum(((float(rows[b, r, d]) - float(cols[b, c, d])) / float(scale[d if len(scale) > 1 else 0])) ** 2
                              for d in range(D))
                term = float(col_a[b, c]) - (0.0 if col_sub is None else float(col_sub[b, c]))
                s.append(term - 0.5 * q)
            top = max(s)
            total = math.fsum(math.exp(v - top) for v in s)
            out[b, r] = (0.0 if row_add is None else float(row_add[b, r])) + (top + math.log(total))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,R,C,D,vector_scale", [(1, 1, 1, 1, False), (2, 4, 5, 2, True), (2, 7, 33, 3, False),
                                                  (1, 3, 70, 1, True), (2, 5, 9, 0, True)])
def test_contract_equals_a_loop_over_every_pair(dtype, B, R, C, D, vector_scale):
    rng = np.random.RandomState(B * 1000 + C)
    rows, cols, scale, col_a, col_sub, row_add = _operands(rng, B, R, C, D, dtype, vector_scale)
    for sub, add in ((col_sub, row_add), (None, None), (col_sub, None), (None, row_add)):
        out, flags = contract.pairwise_lse(rows, cols, scale, col_a, sub, add)
        bound = contract.pairwise_lse_bound(rows, cols, scale, col_a, sub, add)
        assert flags == 0 and out.dtype == np.float64 and out.shape == bound.shape == (B, R)
        assert (bound > 0).all() and (bound < 1e-11).all()
        error = np.abs(out - brute_force(rows, cols, scale, col_a, sub, add))
        assert (error <= bound).all(), (error.max(), bound.min())


def test_special_values():
    rng = np.random.RandomState(1)
    B, R, C, D = 3, 4, 6, 2
    rows, cols, scale, col_a, col_sub, row_add = _operands(rng, B, R, C, D)
    clean, flags = contract.pairwise_lse(rows, cols, scale, col_a, col_sub, row_add)
    assert flags == 0 and np.isfinite(clean).all()

    def run(**changed):
        operands = dict(rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add)
        for name, (index, value) in changed.items():
            operands[name] = operands[name].copy()
            operands[name][index] = value
        return contract.pairwise_lse(**operands)

    def others_untouched(out, bad):
        assert np.array_equal(out[~bad], clean[~bad])

    point = np.zeros((B, R), dtype=bool)
    point[1, 2] = True
    row = np.zeros((B, R), dtype=bool)
    row[1] = True
    # an absent column: its term is -inf whatever col_sub holds (a NaN, or the -inf that would make it -inf + inf)
    for sub in (np.nan, -np.inf, np.inf, 0.0):
        out, flags = run(col_a=((1, 3), -np.inf), col_sub=((1, 3), sub))
        assert flags == 0 and np.isfinite(out).all()
        kept = np.arange(C) != 3
        want = contract.pairwise_lse(rows[1:2], cols[1:2, kept], scale, col_a[1:2, kept], col_sub[1:2, kept], row_add[1:2])[0]
        assert (np.abs(out[1] - want[0]) <= contract.pairwise_lse_bound(rows[1:2], cols[1:2, kept], scale, col_a[1:2, kept],
                                                                        col_sub[1:2, kept], row_add[1:2])[0]).all()
        others_untouched(out, row)
    # NaN: in a row point, in its row_add (that point alone), in a column or its weights (the whole batch row), in the scale
    for changed, bad in ((dict(rows=((1, 2, 0), np.nan)), point), (dict(row_add=((1, 2), np.nan)), point),
                         (dict(cols=((1, 3, 1), np.nan)), row), (dict(col_a=((1, 3), np.nan)), row),
                         (dict(col_sub=((1, 3), np.nan)), row), (dict(col_a=((1, 3), np.inf), col_sub=((1, 3), np.inf)), row),
                         (dict(scale=(0, np.nan)), np.ones((B, R), dtype=bool))):
        out, flags = run(**changed)
        assert flags == contract.FLAG_NAN_LOG_WEIGHT, changed
        assert np.isnan(out[bad]).all()
        others_untouched(out, bad)
    # a maximum of +inf: a present column over a denominator without mass, or a weight of +inf
    for changed in (dict(col_sub=((1, 3), -np.inf)), dict(col_a=((1, 3), np.inf))):
        out, flags = run(**changed)
        assert flags == contract.FLAG_DEGENERATE_ROW and (out[row] == np.inf).all()
        others_untouched(out, row)
    # every score -inf: zero weight, no flag — every column absent, or the one row point infinitely far from all of them
    out, flags = run(col_a=((1, slice(None)), -np.inf))
    assert flags == 0 and (out[row] == -np.inf).all()
    others_untouched(out, row)
    out, flags = run(rows=((1, 2, 0), np.inf))
    assert flags == 0 and (out[point] == -np.inf).all()
    others_untouched(out, point)
    # NaN wins over +inf, and both bits are raised when different points have them
    out, flags = run(col_sub=((1, 3), -np.inf), row_add=((1, 2), np.nan), col_a=((2, 0), np.nan))
    assert flags == contract.FLAG_NAN_LOG_WEIGHT | contract.FLAG_DEGENERATE_ROW
    assert np.isnan(out[1, 2]) and (out[1, [0, 1, 3]] == np.inf).all() and np.isnan(out[2]).all()
    assert np.array_equal(out[0], clean[0])
    assert (contract.pairwise_lse_bound(rows, cols, scale, np.where(row[:, :1], -np.inf, col_a), col_sub, row_add)[1] == 0).all()


def test_row_points_batch_rows_and_columns_are_independent():
    rng = np.random.RandomState(4)
    B, R, C, D = 3, 11, 29, 2
    rows, cols, scale, col_a, col_sub, row_add = _operands(rng, B, R, C, D)
    out, _ = contract.pairwise_lse(rows, cols, scale, col_a, col_sub, row_add)
    bound = contract.pairwise_lse_bound(rows, cols, scale, col_a, col_sub, row_add)
    perm = rng.permutation(R)
    moved, _ = contract.pairwise_lse(rows[:, perm], cols, scale, col_a, col_sub, row_add[:, perm])
    np.testing.assert_array_equal(moved, out[:, perm])
    order = rng.permutation(B)
    moved, _ = contract.pairwise_lse(rows[order], cols[order], scale, col_a[order], col_sub[order], row_add[order])
    np.testing.assert_array_equal(moved, out[order])
    perm = rng.permutation(C)
    moved, _ = contract.pairwise_lse(rows, cols[:, perm], scale, col_a[:, perm], col_sub[:, perm], row_add)
    assert (np.abs(moved - out) <= bound).all()
    np.testing.assert_array_equal(contract.pairwise_lse_bound(rows, cols[:, perm], scale, col_a[:, perm], col_sub[:, perm],
                                                              row_add), bound)


def _scalar_logsumexp(values, axis):
    top = values.max(axis=axis, keepdims=True)
    return (top + np.log(np.exp(values - top).sum(axis=axis, keepdims=True))).squeeze(axis)


def test_marginal_pass_equals_the_recursion_through_explicit_matrices():
    rng = np.random.RandomState(7)
    T, B, K, d = 3, 2, 5, 2
    A = 0.8 * np.eye(d) + 0.1 * rng.randn(d, d)
    scale = np.array([0.7, 1.1])
    x = [rng.randn(B, K, d) for _ in range(T)]
    log_w = [rng.randn(B, K) - 3.0 for _ in range(T)]          # (not normalised)
    got, tolerance = contract.marginal_pass(x, log_w, lambda t: x[t] @ A.T, scale, return_tolerance=True)
    assert len(got) == T and all(g.shape == (B, K) and g.dtype == np.float64 for g in got)
    for b in range(B):
        w = np.exp(log_w[T - 1][b])
        smoothed = w / w.sum()
        np.testing.assert_allclose(np.exp(got[T - 1][b]), smoothed, rtol=1e-13)
        for t in range(T - 2, -1, -1):
            w = np.exp(log_w[t][b]) / np.exp(log_w[t][b]).sum()
            # F[i,j] = f(x[t+1][j] | x[t][i]) with its normalising constant, which has to cancel
            diff = (x[t + 1][b][None, :, :] - (x[t][b] @ A.T)[:, None, :]) / scale
            F = np.exp(-0.5 * (diff ** 2).sum(-1)) / np.prod(scale * np.sqrt(2 * np.pi))
            smoothed = w * (F @ (smoothed / (w @ F)))
            np.testing.assert_allclose(np.exp(got[t][b]), smoothed, rtol=1e-12)
    for t in range(T):
        assert np.abs(_scalar_logsumexp(got[t], 1)).max() <= 1e-12
        assert (tolerance[t] > 0).all() and tolerance[t].max() < 1e-12
    assert tolerance[0].min() > tolerance[T - 1].max()          # it accumulates


def test_every_steps_weights_sum_to_one_on_the_long_scalar_problem():
    """A bootstrap filter in NumPy on the random walk of test_smoothed_posterior_against_the_exact_smoother (T cut to 30,
    K to 100), then the contract's recursion: |logsumexp| <= 1e-12 at every step, and the smoothed weights differ from the
    filter's."""
    rng = np.random.RandomState(0)
    T, K, B = 30, 100, 2
    y = 40 * (np.sin(np.linspace(0, 3 * np.pi, 100)) + 0.2 * rng.randn(100))[:T]
    q, r = 25.0, 64.0
    x, log_w = [], []
    particles = 10.0 * rng.randn(B, K)
    for t in range(T):
        if t > 0:
            w = np.exp(log_w[-1] - log_w[-1].max(axis=1, keepdims=True))
            index = np.stack([rng.choice(K, size=K, p=w[b] / w[b].sum()) for b in range(B)])
            particles = np.take_along_axis(x[-1], index, 1) + np.sqrt(q) * rng.randn(B, K)
        x.append(particles)
        log_w.append(-0.5 * (y[t] - particles) ** 2 / r)
    smoothed = contract.marginal_pass(x, log_w, lambda t: x[t], np.array([np.sqrt(q)]))
    for t in range(T):
        assert np.abs(_scalar_logsumexp(smoothed[t], 1)).max() <= 1e-12, t
    assert np.abs(smoothed[0] - (log_w[0] - _scalar_logsumexp(log_w[0], 1)[:, None])).max() > 0.1


def test_the_abi_rejects_bad_arguments_before_any_launch():
    """NULL pointers, negative sizes, a bad dtype tag or scale stride and row points without columns give status 1, a
    distance term wider than 256 values or sizes beyond 2^30 status 2, an empty problem is a no-op — no GPU needed."""
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    view = _lib.View3(16, 4, 1, 1)
    ref = ctypes.byref(view)

    def call(rows=ref, cols=ref, scale=16, scale_stride=0, col_a=16, col_sub=None, row_add=None, out=16, B=1, R=2, C=4, D=1,
             dtype=0):
        return lib.aesmc_pairwise_lse(dtype, rows, cols, scale, scale_stride, col_a, col_sub, row_add, out, None, B, R, C, D,
                                      None)

    assert call(col_a=None) == 1 and call(out=None) == 1
    assert call(rows=None) == 1 and call(cols=None) == 1 and call(scale=None) == 1
    assert call(rows=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1 and call(cols=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1
    assert call(B=-1) == 1 and call(R=-1) == 1 and call(C=-1) == 1 and call(D=-1) == 1
    assert call(dtype=7) == 1 and call(dtype=-1) == 1 and call(scale_stride=2) == 1 and call(scale_stride=-1) == 1
    assert call(C=0) == 1                                            # row points and nothing to sum over
    assert call(D=257) == 2 and call(R=1 << 30) == 2 and call(C=1 << 31) == 2 and call(B=1 << 31) == 2
    assert call(B=1 << 29, R=64) == 2                                # more workgroups than a grid holds
    assert call(B=0) == 0 and call(R=0) == 0 and call(B=0, D=257) == 0 and call(R=0, C=0) == 0
    assert call(rows=None, cols=None, scale=None, D=0, B=0) == 0     # the D == 0 form takes NULL terms
    assert call(D=257, col_a=None) == 1                              # an invalid argument is reported before the shape
    assert lib.aesmc_version() == 501                                # additive: the ABI's version stays


# ---- the host logic on the oracle provider -----------------------------------------------------------------------------
class MarginalOracle(OracleKernels):
    """The suite's oracle provider plus `pairwise_lse` from the NumPy contract, rounded to the operands' dtype."""

    def __init__(self):
        super().__init__()
        self.calls = []

    @staticmethod
    def pairwise_lse_covers(rows, cols, scale, col_a, col_sub=None, row_add=None):
        from aesmc_amd import _kernels
        return _kernels.HipKernels.pairwise_lse_covers(rows, cols, scale, col_a, col_sub, row_add)

    def pairwise_lse(self, rows, cols, scale, col_a, col_sub=None, row_add=None):
        if not self.pairwise_lse_covers(rows, cols, scale, col_a, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_lse does not take these operands (see pairwise_lse_covers)")
        n = lambda t: None if t is None else t.detach().numpy()
        self.calls.append(dict(rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add))
        out, flags = contract.pairwise_lse(n(rows), n(cols), n(scale), n(col_a), n(col_sub), n(row_add))
        self._flags |= flags
        return torch.from_numpy(out).to(col_a.dtype)


@pytest.fixture
def marginal_backend():
    from aesmc_amd import _kernels
    provider = MarginalOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _filtered(affine=False, dtype=torch.float64, T=5, B=3, K=24, d=2):
    from aesmc_amd import inference
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(d, dtype=dtype, affine=affine).tune_proposal()
    observations = model.simulate(T, B, seed=1)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                          return_latents=False, return_original_latents=True, return_log_weights=True)
    return model, observations, out["original_latents"], out["log_weights"]


@pytest.mark.parametrize("affine", [False, True])
def test_marginal_log_weights_equals_the_numpy_marginal_pass(marginal_backend, affine):
    from aesmc_amd import _lazy, smoothing
    model, observations, latents, log_weights = _filtered(affine=affine)
    T, (B, K, d) = len(latents), latents[0].shape
    got = smoothing.marginal_log_weights(latents, log_weights, model.transition, observations=observations)
    A = model.A.detach().numpy()
    x = [_lazy.real(latent).detach().numpy() for latent in latents]
    w = [weight.detach().numpy() for weight in log_weights]
    scale = np.array([float(model.transition_scale)])
    want, tolerance = contract.marginal_pass(x, w, lambda t: x[t] @ A.T, scale, return_tolerance=True)
    assert len(got) == T
    for t in range(T):
        assert got[t].shape == (B, K) and got[t].dtype == log_weights[t].dtype and not got[t].requires_grad
        if affine:      # (the affine location is the C oracle's fma chain: a last place of the location, not of the sum)
            np.testing.assert_allclose(got[t].numpy(), want[t], rtol=0, atol=1e-12)
        else:
            assert (np.abs(got[t].numpy() - want[t]) <= tolerance[t]).all(), t
        assert np.abs(torch.logsumexp(got[t], dim=1).numpy()).max() <= 1e-12
    # two provider calls per step, last step first: the denominators, then the weights
    calls = marginal_backend.calls
    assert len(calls) == 2 * (T - 1)
    for number, t in enumerate(range(T - 2, -1, -1)):
        den, weights = calls[2 * number], calls[2 * number + 1]
        loc = x[t] @ A.T
        assert np.array_equal(den["rows"].numpy(), x[t + 1]) and np.allclose(den["cols"].numpy(), loc, rtol=0, atol=1e-14)
        assert np.array_equal(den["col_a"].numpy(), w[t]) and den["col_sub"] is None and den["row_add"] is None
        assert weights["rows"] is den["cols"] and weights["cols"] is den["rows"]
        assert torch.equal(weights["col_a"], got[t + 1]) and np.array_equal(weights["row_add"].numpy(), w[t])
        assert weights["col_sub"].shape == (B, K) and weights["col_sub"].dtype == got[t].dtype
        assert tuple(den["scale"].shape) == tuple(weights["scale"].shape) == (1,)
        assert np.array_equal(weights["col_sub"].numpy(), contract.pairwise_lse(x[t + 1], den["cols"].numpy(), scale, w[t])[0])


def test_it_is_deterministic_and_leaves_the_random_states_alone(marginal_backend):
    from aesmc_amd import distributed, smoothing
    model, observations, latents, log_weights = _filtered()
    np.random.seed(11)
    torch.manual_seed(3)
    numpy_before, torch_before = np.random.get_state(), torch.get_rng_state()
    first = smoothing.marginal_log_weights(latents, log_weights, model.transition)
    numpy_after = np.random.get_state()
    assert numpy_before[0] == numpy_after[0] and (numpy_before[1] == numpy_after[1]).all() and \
        numpy_before[2:] == numpy_after[2:]
    assert torch.equal(torch_before, torch.get_rng_state())
    again = smoothing.marginal_log_weights(latents, log_weights, model.transition)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # a constant added to a step's log-weights cancels (up to the rounding of the sums it moves)
    shifted = [w + 5.0 for w in log_weights]
    moved = smoothing.marginal_log_weights(latents, shifted, model.transition)
    assert all(torch.allclose(a, b, rtol=0, atol=1e-12) for a, b in zip(first, moved))
    with distributed.shard_scope(2 * latents[0].shape[0], 0, 2):      # rows are independent: nothing to refuse
        sharded = smoothing.marginal_log_weights(latents, log_weights, model.transition)
    assert all(torch.equal(a, b) for a, b in zip(first, sharded))


def test_refusals(marginal_backend):
    from aesmc_amd import smoothing, state
    full = state.BatchShapeMode.FULLY_EXPANDED
    model, observations, latents, log_weights = _filtered()
    T, (B, K, d) = len(latents), latents[0].shape
    run = lambda transition: smoothing.marginal_log_weights(latents, log_weights, transition)
    tag = lambda dist, mode=full: state.set_batch_shape_mode(dist, mode)
    loc = lambda previous_latents: previous_latents[-1] @ model.A.t()
    with pytest.raises(NotImplementedError, match="dict latents"):
        smoothing.marginal_log_weights([{"x": x} for x in latents], log_weights, model.transition)
    with pytest.raises(NotImplementedError, match="Laplace"):
        run(lambda previous_latents=None, **kw: tag(torch.distributions.Laplace(loc(previous_latents), 1.0)))
    with pytest.raises(NotImplementedError, match="Independent"):
        run(lambda previous_latents=None, **kw: tag(torch.distributions.Independent(Normal(loc(previous_latents), 1.0), 1)))
    with pytest.raises(NotImplementedError, match="dict"):
        run(lambda previous_latents=None, **kw: {"x": tag(Normal(loc(previous_latents), 1.0))})
    with pytest.raises(NotImplementedError, match="particle-dependent"):
        run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents), torch.ones(B, K, d, dtype=torch.float64))))
    with pytest.raises(NotImplementedError, match="FULLY_EXPANDED"):
        run(lambda previous_latents=None, **kw: tag(Normal(torch.zeros(d, dtype=torch.float64), 1.0),
                                                    state.BatchShapeMode.NOT_EXPANDED))
    with pytest.raises(NotImplementedError, match="location of shape"):
        run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents)[..., :1], 1.0)))
    wide = [torch.zeros(B, K, 257, dtype=torch.float64) for _ in range(T)]
    with pytest.raises(NotImplementedError, match="D > 256"):
        smoothing.marginal_log_weights(wide, log_weights, lambda previous_latents=None, **kw: tag(Normal(previous_latents[-1], 1.0)))
    with pytest.raises(ValueError, match="equally long"):
        smoothing.marginal_log_weights(latents, log_weights[:-1], model.transition)
    with pytest.raises(ValueError, match="equally long"):
        smoothing.marginal_log_weights([], [], model.transition)
    with pytest.raises(ValueError, match="does not take these operands"):      # one dtype throughout
        smoothing.marginal_log_weights(latents, [w.float() for w in log_weights], model.transition)
    assert marginal_backend.read_flags(None) == 0
    # a per-dimension scale is covered, and the transition is handed what backward_simulate hands it
    per_dim = torch.tensor([0.5, 2.0], dtype=torch.float64)
    seen = []

    def transition(previous_latents=None, time=None, previous_observations=None):
        seen.append((len(previous_latents), time, len(previous_observations)))
        assert all(type(x) is torch.Tensor for x in previous_latents)
        return tag(Normal(loc(previous_latents), per_dim))

    out = smoothing.marginal_log_weights(latents, log_weights, transition, observations=observations)
    assert tuple(marginal_backend.calls[-1]["scale"].shape) == (d,) and out[0].shape == (B, K)
    assert seen == [(t + 1, t + 1, t + 1) for t in range(T - 2, -1, -1)]
    # a single timestep: the normalised filter weights and no call
    before = len(marginal_backend.calls)
    one = smoothing.marginal_log_weights(latents[:1], log_weights[:1], model.transition)
    assert len(one) == 1 and len(marginal_backend.calls) == before
    first = log_weights[0].detach()
    assert not one[0].requires_grad
    np.testing.assert_allclose(one[0].numpy(), (first - torch.logsumexp(first, 1, keepdim=True)).numpy(), rtol=0, atol=1e-14)


def test_bad_rows_are_raised_once_at_the_end(marginal_backend):
    from aesmc_amd import smoothing
    model, observations, latents, log_weights = _filtered()
    T = len(latents)
    poisoned = [w.clone() for w in log_weights]
    poisoned[1][0, 3] = float("nan")
    with pytest.raises(FloatingPointError):
        smoothing.marginal_log_weights(latents, poisoned, model.transition)
    assert len(marginal_backend.calls) == 2 * (T - 1)          # every step ran: the flags are read once, at the end
    # a step whose particles carry no weight: nothing reaches the particles after it — denominators without mass
    dead = [w.clone() for w in log_weights]
    dead[2][1] = -float("inf")
    with pytest.raises(RuntimeError, match="no finite maximum"):
        smoothing.marginal_log_weights(latents, dead, model.transition)
    assert marginal_backend.read_flags(None) == 0      # nothing is left behind for the next call
    # single particles of zero weight are no error: they keep zero weight
    sparse = [w.clone() for w in log_weights]
    sparse[2][1, :5] = -float("inf")
    out = smoothing.marginal_log_weights(latents, sparse, model.transition)
    assert (out[2][1, :5] == -float("inf")).all() and torch.isfinite(out[2][1, 5:]).all()
    assert all(torch.logsumexp(w, dim=1).abs().max() <= 1e-12 for w in out)


def test_marginal_smooth_is_infer_followed_by_marginal_log_weights(marginal_backend):
    import aesmc_amd
    from aesmc_amd import inference, smoothing
    from aesmc_amd.testing.models import LgssmNd
    assert aesmc_amd.smoothing is smoothing
    model = LgssmNd(2, dtype=torch.float64).tune_proposal()
    observations = model.simulate(4, 3, seed=1)
    torch.manual_seed(9)
    np.random.seed(9)
    latents, smoothed, log_z = smoothing.marginal_smooth(observations, model.initial, model.transition, model.emission,
                                                         model.proposal, 16)
    torch.manual_seed(9)
    np.random.seed(9)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 16,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want = smoothing.marginal_log_weights(out["original_latents"], out["log_weights"], model.transition,
                                          observations=observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"])
    assert len(smoothed) == 4 and all(torch.equal(a, b) for a, b in zip(smoothed, want))
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(latents, out["original_latents"]))
    assert smoothed[0].shape == (3, 16)


def test_backward_simulation_frequencies_are_the_marginal_weights():
    """The two contracts against each other: over M = 20 000 backward-simulated trajectories, the number that pass through
    stored particle k at step t lies within 5 sigma + 1 of M exp(marginal log-weight) — at every step, for every
    particle (B = 2, K = 16, T = 4)."""
    rng = np.random.RandomState(12)
    T, B, K, d, M = 4, 2, 16, 2, 20000
    A = np.array([[0.9, 0.1], [-0.1, 0.8]])
    scale = np.array([0.8, 1.2])
    x = [rng.randn(B, K, d) for _ in range(T)]
    log_w = [rng.randn(B, K) for _ in range(T)]
    locations = lambda t: x[t] @ A.T
    smoothed = contract.marginal_pass(x, log_w, locations, scale)
    _, indices = contract.backward_pass(x, log_w, locations, scale, [rng.rand(B, M) for _ in range(T)])
    for t in range(T):
        p = np.exp(smoothed[t])
        for b in range(B):
            counts = np.bincount(indices[t][b], minlength=K)
            sigma = np.sqrt(M * p[b] * (1 - p[b]))
            assert (np.abs(counts - M * p[b]) <= 5 * sigma + 1).all(), (t, b, counts, M * p[b])
