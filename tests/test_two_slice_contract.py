"""CPU checks of the two-slice particle smoother: the NumPy contract of aesmc_pairwise_mean (aesmc_amd/testing/smoothing.py)
against a loop over every (row point, column) pair, its conventions for special values, the backward recursion against
explicit [K,K] matrices, the two marginalisation identities, the ABI's argument checks, and the host logic of
`aesmc_amd.smoothing.two_slice_expectation` / `two_slice_smooth` on a provider that adds `pairwise_mean` and `pairwise_lse`
from the contract to the suite's oracle provider."""
import math

import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import smoothing as contract
from tests.oracle_provider import OracleKernels


def _operands(rng, B, R, C, D, P, dtype=np.float64, vector_scale=True):
    rows, cols = rng.randn(B, R, D).astype(dtype), rng.randn(B, C, D).astype(dtype)
    scale = (0.5 + rng.rand(D if vector_scale else 1)).astype(dtype)
    col_a, col_sub, row_add = (2 * rng.randn(B, C)).astype(dtype), rng.randn(B, C).astype(dtype), rng.randn(B, R).astype(dtype)
    payload = (3 * rng.randn(B, C, P)).astype(dtype)
    return rows, cols, scale, col_a, payload, col_sub, row_add


def brute_force(rows, cols, scale, col_a, payload, col_sub, row_add):
    """One pair at a time in Python floats (IEEE float64): a true division by the scale, math.exp, exact sums (fsum) and a
    true division of the two sums."""
    B, R, D = rows.shape
    C, P = payload.shape[1:]
    out = np.empty((B, R, P))
    for b in range(B):
        for r in range(R):
            s = []
            for c in range(C):
                q = math.fsum(((float(rows[b, r, d]) - float(cols[b, c, d])) / float(scale[d if len(scale) > 1 else 0])) ** 2
                              for d in range(D))
                term = float(col_a[b, c]) - (0.0 if col_sub is None else float(col_sub[b, c]))
                s.append(term - 0.5 * q)
            top = max(s)
            e = [math.exp(v - top) for v in s]
            total = math.fsum(e)
            for p in range(P):
                out[b, r, p] = math.fsum(e[c] * float(payload[b, c, p]) for c in range(C)) / total
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,R,C,D,P,vector_scale", [(1, 1, 1, 1, 1, False), (2, 4, 5, 2, 3, True), (2, 7, 33, 3, 1, False),
                                                    (1, 3, 70, 1, 17, True), (2, 5, 9, 0, 2, True)])
def test_contract_equals_a_loop_over_every_pair(dtype, B, R, C, D, P, vector_scale):
    rng = np.random.RandomState(B * 1000 + C)
    rows, cols, scale, col_a, payload, col_sub, row_add = _operands(rng, B, R, C, D, P, dtype, vector_scale)
    for sub, add in ((col_sub, row_add), (None, None), (col_sub, None), (None, row_add)):
        out, lse, flags = contract.pairwise_mean(rows, cols, scale, col_a, payload, sub, add)
        bound = contract.pairwise_mean_bound(rows, cols, scale, col_a, payload, sub, add)
        assert flags == 0 and out.dtype == lse.dtype == np.float64 and out.shape == bound.shape == (B, R, P)
        assert (bound > 0).all() and (bound < 1e-10).all()
        error = np.abs(out - brute_force(rows, cols, scale, col_a, payload, sub, add))
        assert (error <= bound).all(), (error.max(), bound.min())
        assert np.array_equal(lse, contract.pairwise_lse(rows, cols, scale, col_a, sub, add)[0])
    bound = contract.pairwise_mean_bound(rows, cols, scale, col_a, payload, col_sub, row_add)
    # a payload of any trailing shape is flattened; a [B,C] one has one value per column
    shaped, _, _ = contract.pairwise_mean(rows, cols, scale, col_a, payload.reshape(B, C, P, 1), col_sub, row_add)
    assert np.array_equal(shaped, contract.pairwise_mean(rows, cols, scale, col_a, payload, col_sub, row_add)[0])
    flat, _, _ = contract.pairwise_mean(rows, cols, scale, col_a, payload[:, :, 0], col_sub, row_add)
    assert flat.shape == (B, R, 1) and (np.abs(flat[:, :, 0] - shaped[:, :, 0]) <= bound[:, :, 0]).all()      # (NumPy's order of the C additions depends on P)
    with pytest.raises(ValueError, match="one payload per column"):
        contract.pairwise_mean(rows, cols, scale, col_a, payload[:, :-1] if C > 1 else payload[:, :0], col_sub, row_add)


def test_special_values():
    rng = np.random.RandomState(1)
    B, R, C, D, P = 3, 4, 6, 2, 3
    rows, cols, scale, col_a, payload, col_sub, row_add = _operands(rng, B, R, C, D, P)
    clean, clean_lse, flags = contract.pairwise_mean(rows, cols, scale, col_a, payload, col_sub, row_add)
    assert flags == 0 and np.isfinite(clean).all()

    def run(**changed):
        operands = dict(rows=rows, cols=cols, scale=scale, col_a=col_a, payload=payload, col_sub=col_sub, row_add=row_add)
        for name, (index, value) in changed.items():
            operands[name] = operands[name].copy()
            operands[name][index] = value
        return contract.pairwise_mean(**operands)

    def others_untouched(out, lse, bad):
        assert np.array_equal(out[~bad], clean[~bad]) and np.array_equal(lse[~bad], clean_lse[~bad])

    point = np.zeros((B, R), dtype=bool)
    point[1, 2] = True
    row = np.zeros((B, R), dtype=bool)
    row[1] = True
    kept = np.arange(C) != 3
    # an absent column: whatever its payload (and its col_sub) holds never reaches a result — selected, not multiplied
    without = contract.pairwise_mean(rows[1:2], cols[1:2, kept], scale, col_a[1:2, kept], payload[1:2, kept],
                                     col_sub[1:2, kept], row_add[1:2])
    for held in (np.nan, np.inf, -np.inf, 1e300):
        out, lse, flags = run(col_a=((1, 3), -np.inf), payload=((1, 3), held), col_sub=((1, 3), np.nan))
        assert flags == 0 and np.isfinite(out).all() and np.isfinite(lse).all()
        assert np.array_equal(out[1], without[0][0]) and np.array_equal(lse[1], without[1][0])
        others_untouched(out, lse, row)
    # NaN: in a row point, in its row_add (that point alone), in a column or its weights (the whole batch row)
    for changed, bad in ((dict(rows=((1, 2, 0), np.nan)), point), (dict(row_add=((1, 2), np.nan)), point),
                         (dict(cols=((1, 3, 1), np.nan)), row), (dict(col_a=((1, 3), np.nan)), row),
                         (dict(col_sub=((1, 3), np.nan)), row), (dict(scale=(0, np.nan)), np.ones((B, R), dtype=bool))):
        out, lse, flags = run(**changed)
        assert flags == contract.FLAG_NAN_LOG_WEIGHT, changed
        assert np.isnan(out[bad]).all() and np.isnan(lse[bad]).all()
        others_untouched(out, lse, bad)
    # a largest score of +inf: the flag, lse +inf, no weights to average with
    for changed in (dict(col_sub=((1, 3), -np.inf)), dict(col_a=((1, 3), np.inf))):
        out, lse, flags = run(**changed)
        assert flags == contract.FLAG_DEGENERATE_ROW and (lse[row] == np.inf).all() and np.isnan(out[row]).all()
        others_untouched(out, lse, row)
    # every score -inf: out 0, lse -inf and no flag — every column absent, or the one row point infinitely far from all
    out, lse, flags = run(col_a=((1, slice(None)), -np.inf), payload=((1, 0), np.nan))
    assert flags == 0 and (out[row] == 0).all() and (lse[row] == -np.inf).all()
    others_untouched(out, lse, row)
    out, lse, flags = run(rows=((1, 2, 0), np.inf))
    assert flags == 0 and (out[point] == 0).all() and (lse[point] == -np.inf).all()
    others_untouched(out, lse, point)
    # the bound is zero where the result is a convention
    bound = contract.pairwise_mean_bound(rows, cols, scale, np.where(row[:, :1], -np.inf, col_a), payload, col_sub, row_add)
    assert (bound[1] == 0).all() and (bound[0] > 0).all()


def test_row_points_and_batch_rows_are_independent():
    rng = np.random.RandomState(4)
    B, R, C, D, P = 3, 11, 29, 2, 4
    rows, cols, scale, col_a, payload, col_sub, row_add = _operands(rng, B, R, C, D, P)
    out, lse, _ = contract.pairwise_mean(rows, cols, scale, col_a, payload, col_sub, row_add)
    bound = contract.pairwise_mean_bound(rows, cols, scale, col_a, payload, col_sub, row_add)
    perm = rng.permutation(R)
    moved, _, _ = contract.pairwise_mean(rows[:, perm], cols, scale, col_a, payload, col_sub, row_add[:, perm])
    np.testing.assert_array_equal(moved, out[:, perm])
    order = rng.permutation(B)
    moved, _, _ = contract.pairwise_mean(rows[order], cols[order], scale, col_a[order], payload[order], col_sub[order],
                                         row_add[order])
    np.testing.assert_array_equal(moved, out[order])
    perm = rng.permutation(C)
    moved, _, _ = contract.pairwise_mean(rows, cols[:, perm], scale, col_a[:, perm], payload[:, perm], col_sub[:, perm], row_add)
    assert (np.abs(moved - out) <= bound).all()
    # a constant payload comes back whatever the weights are, and the mean is linear in the payload
    ones, _, _ = contract.pairwise_mean(rows, cols, scale, col_a, np.full((B, C, 1), 2.5), col_sub, row_add)
    assert np.abs(ones - 2.5).max() <= 1e-14


def _logsumexp(values, axis):
    top = values.max(axis=axis, keepdims=True)
    return (top + np.log(np.exp(values - top).sum(axis=axis, keepdims=True))).squeeze(axis)


def _random_problem(seed, T=3, B=2, K=5, d=2):
    rng = np.random.RandomState(seed)
    A = 0.8 * np.eye(d) + 0.1 * rng.randn(d, d)
    scale = np.array([0.7, 1.1])[:d]
    x = [rng.randn(B, K, d) for _ in range(T)]
    log_w = [rng.randn(B, K) - 3.0 for _ in range(T)]          # (not normalised)
    return A, scale, x, log_w


def test_two_slice_pass_equals_the_recursion_through_explicit_matrices():
    T, B, K, d = 3, 2, 5, 2
    A, scale, x, log_w = _random_problem(7, T, B, K, d)
    square = lambda t, v: np.concatenate([v, v ** 2, np.ones(v.shape[:2] + (1,))], axis=-1)          # P = 2 d + 1
    shifted = lambda t, v: v[..., :1] + t                                                             # Q = 1, uses the time
    for previous, following in ((None, None), (square, shifted)):
        (got, smoothed, (tolerance, smoothed_tolerance)) = contract.two_slice_pass(
            x, log_w, lambda t: x[t] @ A.T, scale, previous, following, return_tolerance=True)
        marginal, marginal_tolerance = contract.marginal_pass(x, log_w, lambda t: x[t] @ A.T, scale, return_tolerance=True)
        assert len(got) == T - 1 and len(smoothed) == T
        assert all(np.array_equal(a, b) for a, b in zip(smoothed, marginal))          # the same recursion, the same bits
        assert all(np.array_equal(a, b) for a, b in zip(smoothed_tolerance, marginal_tolerance))
        for b in range(B):
            w = np.exp(log_w[T - 1][b])
            after = w / w.sum()
            for t in range(T - 2, -1, -1):
                w = np.exp(log_w[t][b]) / np.exp(log_w[t][b]).sum()
                # F[i,j] = f(x[t+1][j] | x[t][i]) with its normalising constant, which has to cancel
                diff = (x[t + 1][b][None, :, :] - (x[t][b] @ A.T)[:, None, :]) / scale
                F = np.exp(-0.5 * (diff ** 2).sum(-1)) / np.prod(scale * np.sqrt(2 * np.pi))
                W = w[:, None] * F * (after / (w @ F))[None, :]                        # the two-slice weights [i,j]
                assert abs(W.sum() - 1) < 1e-12
                f = x[t][b] if previous is None else previous(t, x[t])[b]
                g = x[t + 1][b] if following is None else following(t + 1, x[t + 1])[b]
                want = np.einsum("ij,jq,ip->qp", W, g, f)
                assert got[t][b].shape == want.shape and got[t].dtype == np.float64
                np.testing.assert_allclose(got[t][b], want, rtol=1e-11, atol=1e-13)
                after = W.sum(axis=1)
        for t in range(T - 1):
            assert (tolerance[t] > 0).all() and tolerance[t].max() < 1e-11


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_two_marginalisation_identities(dtype):
    """following = 1 gives the means of `previous` under smoothed[t], previous = 1 those of `following` under
    smoothed[t + 1] — within the tolerance the pass returns, plus the marginal weights' own (the means are formed from
    log-weights that carry it)."""
    T, B, K, d = 4, 2, 9, 2
    A, scale, x, log_w = _random_problem(11, T, B, K, d)
    x, log_w, scale = [v.astype(dtype) for v in x], [v.astype(dtype) for v in log_w], scale.astype(dtype)
    ones = lambda t, v: np.ones(v.shape[:2] + (1,), dtype=v.dtype)
    locations = lambda t: (x[t].astype(np.float64) @ A.T).astype(dtype)
    for previous, following in ((None, ones), (ones, None)):
        got, smoothed, (tolerance, smoothed_tolerance) = contract.two_slice_pass(x, log_w, locations, scale, previous,
                                                                                 following, return_tolerance=True)
        for t in range(T - 1):
            at = t if following is ones else t + 1
            w = np.exp(smoothed[at].astype(np.float64))
            mean = np.einsum("bk,bkd->bd", w, x[at].astype(np.float64))
            slack = np.einsum("bk,bkd->bd", w * 2 * smoothed_tolerance[at], np.abs(x[at]).astype(np.float64))
            mine = got[t].astype(np.float64).reshape(B, d)
            assert (np.abs(mine - mean) <= tolerance[t].reshape(B, d) + slack + 1e-15).all(), (t, mine, mean)


def test_the_abi_rejects_bad_arguments_before_any_launch():
    """aesmc_pairwise_lse's checks in its order with its statuses, and P < 1 / a NULL payload or out status 1, P > 256
    status 2 — no GPU needed."""
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    view = _lib.View3(16, 4, 1, 1)
    ref = ctypes.byref(view)

    def call(rows=ref, cols=ref, scale=16, scale_stride=0, col_a=16, col_sub=None, row_add=None, payload=ref, out=16, lse=16,
             B=1, R=2, C=4, D=1, P=3, dtype=0):
        return lib.aesmc_pairwise_mean(dtype, rows, cols, scale, scale_stride, col_a, col_sub, row_add, payload, out, lse,
                                       None, B, R, C, D, P, None)

    assert call(col_a=None) == 1 and call(out=None) == 1 and call(payload=None) == 1
    assert call(payload=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1
    assert call(rows=None) == 1 and call(cols=None) == 1 and call(scale=None) == 1
    assert call(rows=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1 and call(cols=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1
    assert call(B=-1) == 1 and call(R=-1) == 1 and call(C=-1) == 1 and call(D=-1) == 1
    assert call(P=0) == 1 and call(P=-1) == 1 and call(P=0, B=0) == 1
    assert call(dtype=7) == 1 and call(dtype=-1) == 1 and call(scale_stride=2) == 1 and call(scale_stride=-1) == 1
    assert call(C=0) == 1                                            # row points and nothing to average over
    assert call(P=257) == 2 and call(D=257) == 2 and call(R=1 << 30) == 2 and call(C=1 << 31) == 2 and call(B=1 << 31) == 2
    assert call(B=1 << 29, R=64) == 2                                # more workgroups than a grid holds
    assert call(B=0) == 0 and call(R=0) == 0 and call(B=0, D=257) == 0 and call(B=0, P=257) == 0 and call(R=0, C=0) == 0
    assert call(rows=None, cols=None, scale=None, D=0, B=0) == 0     # the D == 0 form takes NULL terms
    assert call(B=0, lse=None) == 0                                  # lse_out is optional
    assert call(P=257, col_a=None) == 1 and call(D=257, payload=None) == 1      # invalid is reported before unsupported
    for form in (1, 2, 3, 0):
        assert lib.aesmc_test_set_pairwise_mean_form(form) == 0
    assert lib.aesmc_test_set_pairwise_mean_form(4) == 1 and lib.aesmc_test_set_pairwise_mean_form(-1) == 1
    assert lib.aesmc_version() == 501                                # additive: the ABI's version stays


# ---- the host logic on the oracle provider -----------------------------------------------------------------------------
class TwoSliceOracle(OracleKernels):
    """The suite's oracle provider plus `pairwise_lse` and `pairwise_mean` from the NumPy contract, rounded to the
    operands' dtype."""

    def __init__(self):
        super().__init__()
        self.calls = []

    @staticmethod
    def pairwise_lse_covers(*operands):
        from aesmc_amd import _kernels
        return _kernels.HipKernels.pairwise_lse_covers(*operands)

    @staticmethod
    def pairwise_mean_covers(*operands):
        from aesmc_amd import _kernels
        return _kernels.HipKernels.pairwise_mean_covers(*operands)

    def pairwise_lse(self, rows, cols, scale, col_a, col_sub=None, row_add=None):
        if not self.pairwise_lse_covers(rows, cols, scale, col_a, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_lse does not take these operands (see pairwise_lse_covers)")
        n = lambda t: None if t is None else t.detach().numpy()
        self.calls.append(dict(kernel="lse", rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add))
        out, flags = contract.pairwise_lse(n(rows), n(cols), n(scale), n(col_a), n(col_sub), n(row_add))
        self._flags |= flags
        return torch.from_numpy(out).to(col_a.dtype)

    def pairwise_mean(self, rows, cols, scale, col_a, payload, col_sub=None, row_add=None):
        if not self.pairwise_mean_covers(rows, cols, scale, col_a, payload, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_mean does not take these operands (see pairwise_mean_covers)")
        n = lambda t: None if t is None else t.detach().numpy()
        self.calls.append(dict(kernel="mean", rows=rows, cols=cols, scale=scale, col_a=col_a, payload=payload,
                               col_sub=col_sub, row_add=row_add))
        out, lse, flags = contract.pairwise_mean(n(rows), n(cols), n(scale), n(col_a), n(payload), n(col_sub), n(row_add))
        self._flags |= flags
        return torch.from_numpy(out).to(col_a.dtype), torch.from_numpy(lse).to(col_a.dtype)


@pytest.fixture
def two_slice_backend():
    from aesmc_amd import _kernels
    provider = TwoSliceOracle()
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


@pytest.mark.parametrize("features", ["latents", "callables"])
def test_two_slice_expectation_equals_the_numpy_two_slice_pass(two_slice_backend, features):
    from aesmc_amd import _lazy, smoothing
    model, observations, latents, log_weights = _filtered()
    T, (B, K, d) = len(latents), latents[0].shape
    seen = {"previous": [], "following": []}

    def previous(time, latent):
        assert type(latent) is torch.Tensor and not latent.requires_grad
        seen["previous"].append(time)
        return torch.stack([latent, latent ** 2], dim=-1)                 # [B,K,d,2]: P = 2 d

    def following(time, latent):
        assert type(latent) is torch.Tensor and not latent.requires_grad
        seen["following"].append(time)
        return latent[..., 0] + time                                      # [B,K]: Q = 1

    functions = (None, None) if features == "latents" else (previous, following)
    got, smoothed = smoothing.two_slice_expectation(latents, log_weights, model.transition, observations=observations,
                                                    previous=functions[0], following=functions[1])
    A = model.A.detach().numpy()
    x = [_lazy.real(latent).detach().numpy() for latent in latents]
    w = [weight.detach().numpy() for weight in log_weights]
    scale = np.array([float(model.transition_scale)])
    numpy_functions = (None, None) if features == "latents" else (
        lambda t, v: np.stack([v, v ** 2], axis=-1), lambda t, v: v[..., 0] + t)
    want, want_smoothed, (tolerance, smoothed_tolerance) = contract.two_slice_pass(
        x, w, lambda t: x[t] @ A.T, scale, numpy_functions[0], numpy_functions[1], return_tolerance=True)
    P, Q = (d, d) if features == "latents" else (2 * d, 1)
    assert len(got) == T - 1 and len(smoothed) == T
    for t in range(T - 1):
        assert got[t].shape == (B, Q, P) and got[t].dtype == latents[0].dtype and not got[t].requires_grad
        assert (np.abs(got[t].numpy() - want[t]) <= tolerance[t]).all(), t
    for t in range(T):
        assert (np.abs(smoothed[t].numpy() - want_smoothed[t]) <= smoothed_tolerance[t]).all(), t
    if features == "callables":          # one call of each per step, last step first, on the stored particles of its time
        assert seen["previous"] == list(range(T - 2, -1, -1)) and seen["following"] == list(range(T - 1, 0, -1))
    # per step: one K23 launch (the means and the denominators), then one K22 launch (the weights)
    calls = two_slice_backend.calls
    assert [call["kernel"] for call in calls] == ["mean", "lse"] * (T - 1)
    for number, t in enumerate(range(T - 2, -1, -1)):
        mean, weights = calls[2 * number], calls[2 * number + 1]
        assert np.array_equal(mean["rows"].numpy(), x[t + 1]) and np.array_equal(mean["col_a"].numpy(), w[t])
        assert mean["col_sub"] is None and mean["row_add"] is None and mean["payload"].shape == (B, K, P)
        assert weights["rows"] is mean["cols"] and weights["cols"] is mean["rows"]
        assert torch.equal(weights["col_a"], smoothed[t + 1]) and np.array_equal(weights["row_add"].numpy(), w[t])
    # its smoothed log-weights are the marginal smoother's on the same provider
    marginal = smoothing.marginal_log_weights(latents, log_weights, model.transition, observations=observations)
    assert all(torch.equal(a, b) for a, b in zip(smoothed, marginal))


def test_it_is_deterministic_and_leaves_the_random_states_alone(two_slice_backend):
    from aesmc_amd import distributed, smoothing
    model, observations, latents, log_weights = _filtered()
    np.random.seed(11)
    torch.manual_seed(3)
    numpy_before, torch_before = np.random.get_state(), torch.get_rng_state()
    first, _ = smoothing.two_slice_expectation(latents, log_weights, model.transition)
    numpy_after = np.random.get_state()
    assert numpy_before[0] == numpy_after[0] and (numpy_before[1] == numpy_after[1]).all() and \
        numpy_before[2:] == numpy_after[2:]
    assert torch.equal(torch_before, torch.get_rng_state())
    again, _ = smoothing.two_slice_expectation(latents, log_weights, model.transition)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    with distributed.shard_scope(2 * latents[0].shape[0], 0, 2):      # rows are independent: nothing to refuse
        sharded, _ = smoothing.two_slice_expectation(latents, log_weights, model.transition)
    assert all(torch.equal(a, b) for a, b in zip(first, sharded))


def test_refusals(two_slice_backend):
    from aesmc_amd import smoothing, state
    full = state.BatchShapeMode.FULLY_EXPANDED
    model, observations, latents, log_weights = _filtered()
    T, (B, K, d) = len(latents), latents[0].shape
    tag = lambda dist, mode=full: state.set_batch_shape_mode(dist, mode)
    loc = lambda previous_latents: previous_latents[-1] @ model.A.t()
    run = lambda transition, **kw: smoothing.two_slice_expectation(latents, log_weights, transition, **kw)
    with pytest.raises(NotImplementedError, match="dict latents"):
        smoothing.two_slice_expectation([{"x": x} for x in latents], log_weights, model.transition)
    with pytest.raises(NotImplementedError, match="Laplace"):
        run(lambda previous_latents=None, **kw: tag(torch.distributions.Laplace(loc(previous_latents), 1.0)))
    with pytest.raises(NotImplementedError, match="particle-dependent"):
        run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents), torch.ones(B, K, d, dtype=torch.float64))))
    with pytest.raises(NotImplementedError, match="P <= 256"):
        run(model.transition, previous=lambda t, x: x.new_zeros(B, K, 257))
    with pytest.raises(NotImplementedError, match="P <= 256"):
        run(model.transition, previous=lambda t, x: x.new_zeros(B, K, 0))
    with pytest.raises(ValueError, match="must return a tensor"):
        run(model.transition, following=lambda t, x: x[:, :-1])
    with pytest.raises(ValueError, match="dtype"):
        run(model.transition, previous=lambda t, x: x.float())
    with pytest.raises(ValueError, match="equally long"):
        smoothing.two_slice_expectation(latents, log_weights[:-1], model.transition)
    with pytest.raises(ValueError, match="equally long"):
        smoothing.two_slice_expectation([], [], model.transition)
    assert two_slice_backend.read_flags(None) == 0
    # Q is not limited; 256 payload values are taken
    out, _ = run(model.transition, previous=lambda t, x: x.new_ones(B, K, 256), following=lambda t, x: x.new_ones(B, K, 300))
    assert out[0].shape == (B, 300, 256) and torch.allclose(out[0], torch.ones_like(out[0]), rtol=0, atol=1e-12)
    # a single timestep: no expectation, the normalised filter weights and no launch
    before = len(two_slice_backend.calls)
    none, one = smoothing.two_slice_expectation(latents[:1], log_weights[:1], model.transition)
    assert none == [] and len(one) == 1 and len(two_slice_backend.calls) == before
    first = log_weights[0].detach()
    np.testing.assert_allclose(one[0].numpy(), (first - torch.logsumexp(first, 1, keepdim=True)).numpy(), rtol=0, atol=1e-14)


def test_bad_rows_are_raised_once_at_the_end(two_slice_backend):
    from aesmc_amd import smoothing
    model, observations, latents, log_weights = _filtered()
    T = len(latents)
    poisoned = [w.clone() for w in log_weights]
    poisoned[1][0, 3] = float("nan")
    with pytest.raises(FloatingPointError):
        smoothing.two_slice_expectation(latents, poisoned, model.transition)
    assert len(two_slice_backend.calls) == 2 * (T - 1)          # every step ran: the flags are read once, at the end
    assert two_slice_backend.read_flags(None) == 0              # ... and are left clear
    dead = [w.clone() for w in log_weights]
    dead[2][1] = -float("inf")
    with pytest.raises(RuntimeError, match="no finite maximum"):
        smoothing.two_slice_expectation(latents, dead, model.transition)
    assert two_slice_backend.read_flags(None) == 0
    # an exception in a feature callable leaves nothing behind either
    def broken(time, latent):
        if time == 0:
            raise KeyError("mine")
        return latent
    with pytest.raises(KeyError):
        smoothing.two_slice_expectation(latents, poisoned, model.transition, previous=broken)
    assert two_slice_backend.read_flags(None) == 0
    # single particles of zero weight are no error: they carry nothing into the expectations
    sparse = [w.clone() for w in log_weights]
    sparse[2][1, :5] = -float("inf")
    out, smoothed = smoothing.two_slice_expectation(latents, sparse, model.transition)
    assert (smoothed[2][1, :5] == -float("inf")).all() and all(torch.isfinite(e).all() for e in out)


def test_two_slice_smooth_is_infer_followed_by_two_slice_expectation(two_slice_backend):
    from aesmc_amd import inference, smoothing
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(2, dtype=torch.float64).tune_proposal()
    observations = model.simulate(4, 3, seed=1)
    square = lambda t, x: x ** 2
    torch.manual_seed(9)
    np.random.seed(9)
    latents, smoothed, expectations, log_z = smoothing.two_slice_smooth(
        observations, model.initial, model.transition, model.emission, model.proposal, 16, previous=square)
    torch.manual_seed(9)
    np.random.seed(9)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 16,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want, want_smoothed = smoothing.two_slice_expectation(out["original_latents"], out["log_weights"], model.transition,
                                                          observations=observations, previous=square)
    marginal = smoothing.marginal_log_weights(out["original_latents"], out["log_weights"], model.transition,
                                              observations=observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"])
    assert len(expectations) == 3 and all(torch.equal(a, b) for a, b in zip(expectations, want))
    assert len(smoothed) == 4 and all(torch.equal(a, b) for a, b in zip(smoothed, want_smoothed))
    assert all(torch.equal(a, b) for a, b in zip(smoothed, marginal))
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(latents, out["original_latents"]))
    assert expectations[0].shape == (3, 2, 2)
