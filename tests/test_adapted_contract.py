"""CPU checks of the fully adapted auxiliary particle filter: the gain algebra (`aesmc_amd.adapted.gains` and its NumPy
contract) against independent formulas, the NumPy contracts of K27 / K28 (aesmc_amd/testing/adapted.py), the restated
filter against the Kalman filter and a NumPy bootstrap filter — where the bounds of the device's statistical test come
from — the ABI's argument checks, and the host logic of `aesmc_amd.adapted.adapted_filter` on a provider that adds the
two launches from their contracts to the suite's oracle provider."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as contract
from tests.oracle_provider import OracleKernels

CASES = [(2, 2, 1.0, 0.5), (3, 2, 0.7, [0.5, 0.2]), (2, 3, [1.0, 0.4], [0.3, 0.5, 0.9]), (1, 1, 0.3, 2.0),
         (5, 4, [0.5, 0.6, 0.7, 0.8, 0.9], 0.25)]


def _weight(D, Dy, seed=0):
    rng = np.random.RandomState(seed)
    return np.eye(Dy, D) + 0.3 * rng.randn(Dy, D)


def _variances(scale, size):
    return np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (size,)) ** 2


@pytest.mark.parametrize("which", ["numpy", "torch"])
@pytest.mark.parametrize("D,Dy,s_f,s_g", CASES)
def test_gains_against_independent_formulas(which, D, Dy, s_f, s_g):
    """base - 1/2 |P mu + o|^2 is the multivariate Normal log-density of y at C mu + d under S (slogdet and solve), to
    1e-12; M mu + r and L L^T are the information-form posterior LgssmNd.tune_proposal documents, to 1e-10."""
    C = _weight(D, Dy, seed=D + 10 * Dy)
    if which == "numpy":
        gain = contract.gains(s_f, C, s_g)
    else:
        from aesmc_amd import adapted
        raw = adapted.gains(torch.tensor(s_f, dtype=torch.float32).double(), torch.from_numpy(C),
                            torch.tensor(s_g, dtype=torch.float64))
        gain = {key: (value.numpy() if torch.is_tensor(value) else value) for key, value in raw.items()}
        s_f = np.asarray(s_f, dtype=np.float32).astype(np.float64)
    rng = np.random.RandomState(3)
    mu, y, d = rng.randn(4, D), rng.randn(4, Dy), rng.randn(Dy)
    S_f, S_g = np.diag(_variances(s_f, D)), np.diag(_variances(s_g, Dy))
    S = C @ S_f @ C.T + S_g
    o, r = contract.row_offsets(gain, y, d)
    for b in range(4):
        residual = y[b] - (C @ mu[b] + d)
        want = -0.5 * (residual @ np.linalg.solve(S, residual) + np.linalg.slogdet(S)[1] + Dy * np.log(2 * np.pi))
        got = gain["base"] - 0.5 * ((gain["P"] @ mu[b] + o[b]) ** 2).sum()
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
        sigma = np.linalg.inv(np.linalg.inv(S_f) + C.T @ np.linalg.inv(S_g) @ C)
        mean = sigma @ (np.linalg.inv(S_f) @ mu[b] + C.T @ np.linalg.inv(S_g) @ (y[b] - d))
        np.testing.assert_allclose(gain["M"] @ mu[b] + r[b], mean, rtol=0, atol=1e-10)
        np.testing.assert_allclose(gain["L"] @ gain["L"].T, sigma, rtol=0, atol=1e-10)
    assert np.array_equal(gain["L"], np.tril(gain["L"]))
    assert gain["P"].shape == (Dy, D) and gain["M"].shape == (D, D)


def test_gains_names_the_covariance_that_fails():
    from aesmc_amd import adapted
    C = torch.eye(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="predictive covariance"):
        adapted.gains(torch.zeros(1, dtype=torch.float64), C, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="optimal proposal's covariance"):
        adapted.gains(torch.zeros(1, dtype=torch.float64), C, torch.ones(1, dtype=torch.float64))


# ---- the two kernels restated ---------------------------------------------------------------------------------------------
def test_kernel_contracts_against_plain_matrix_products():
    rng = np.random.RandomState(0)
    B, K, D, Dy = 3, 7, 4, 3
    loc, eps = rng.randn(B, K, D), rng.randn(B, K, D)
    P, M, L = rng.randn(Dy, D), rng.randn(D, D), np.tril(rng.randn(D, D))
    o, r = rng.randn(B, Dy), rng.randn(B, D)
    out = contract.affine_quadratic_logweight(loc, P, o, -1.5)
    want = -1.5 - 0.5 * ((loc @ P.T + o[:, None, :]) ** 2).sum(axis=2)
    assert (np.abs(out - want) <= contract.affine_quadratic_logweight_bound(loc, P, o, -1.5)).all()
    assert contract.affine_quadratic_logweight_bound(loc, P, o, -1.5).max() < 1e-12
    idx = rng.randint(0, K, size=(B, K))
    draw, flags = contract.adapted_draw(loc, idx, M, r, L + np.triu(np.full((D, D), 99.0), 1), eps)   # nothing above the diagonal is read
    want = r[:, None, :] + np.take_along_axis(loc, idx[:, :, None], axis=1) @ M.T + eps @ L.T
    assert flags == 0 and (np.abs(draw - want) <= contract.adapted_draw_bound(loc, idx, M, r, L, eps)).all()
    same, _ = contract.adapted_draw(loc, None, M, r, L, eps)
    ident, _ = contract.adapted_draw(loc, np.broadcast_to(np.arange(K), (B, K)), M, r, L, eps)
    assert np.array_equal(same, ident)
    # a particle stride of zero; float32 operands round once
    row = loc[:, :1].astype(np.float32)
    wide = contract.affine_quadratic_logweight(np.broadcast_to(row, (B, K, D)), P, o, 0.0)
    assert wide.dtype == np.float32 and (wide == wide[:, :1]).all()
    # an index out of range: NaN there, the flag, everything else unchanged
    bad = idx.copy()
    bad[1, 2], bad[2, 0] = K, -1
    out, flags = contract.adapted_draw(loc, bad, M, r, L, eps)
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE
    hit = np.zeros((B, K), dtype=bool)
    hit[1, 2] = hit[2, 0] = True
    assert np.isnan(out[hit]).all() and np.array_equal(out[~hit], draw[~hit])
    nan_loc = loc.copy()
    nan_loc[0, 3, 1] = np.nan
    lam = contract.affine_quadratic_logweight(nan_loc, P, o, 0.0)
    assert np.isnan(lam[0, 3]) and np.isfinite(np.delete(lam.reshape(-1), 3)).all()


def test_ancestor_index_contract_both_schemes():
    log_w = np.log(np.array([[0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25]]))
    idx, lse, flags, margin = contract.ancestor_index(log_w, np.array([0.5, 0.5]))
    assert flags == 0 and idx.tolist() == [[1, 2, 3, 3], [0, 1, 2, 3]] and margin > 1e-3
    np.testing.assert_allclose(lse, 0.0, atol=1e-15)
    idx, _, _, _ = contract.ancestor_index(log_w, np.array([[0.9, 0.1, 0.9, 0.1], [0.5] * 4]))
    assert idx.tolist() == [[1, 1, 3, 3], [0, 1, 2, 3]]
    bad = log_w.copy()
    bad[0, 1] = np.nan
    bad[1] = -np.inf
    idx, _, flags, _ = contract.ancestor_index(bad, np.array([0.5, 0.5]))
    assert flags == contract.FLAG_NAN_LOG_WEIGHT | contract.FLAG_DEGENERATE_ROW and (idx == 4).all()


# ---- the restated filter ----------------------------------------------------------------------------------------------------
def _lgssm(dim, dtype=torch.float64, **kw):
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(dim, dtype=dtype, **kw)
    return model, model.A.detach().double().numpy(), model.C.detach().double().numpy()


@pytest.mark.parametrize("K", [1, 7, 64])
def test_one_step_is_the_exact_evidence(K):
    model, A, C = _lgssm(3)
    ys = [y.numpy() for y in model.simulate(1, 5, seed=2)]
    rng = np.random.RandomState(K)
    out = contract.adapted_pass(ys, np.zeros(3), np.ones(3), None, 1.0, C, None, 0.5, [rng.randn(5, K, 3)], [])
    _, _, exact = contract.kalman_filter(A, C, 1.0, 0.5, np.zeros(3), np.ones(3), ys)
    np.testing.assert_allclose(out["log_marginal_likelihood"], exact, rtol=0, atol=1e-12)
    from aesmc_amd.testing.models import kalman_log_likelihood
    np.testing.assert_allclose(exact, kalman_log_likelihood(model, [torch.from_numpy(y) for y in ys]), rtol=0, atol=1e-12)


def test_filtered_means_of_step_zero_are_the_kalman_posterior():
    model, A, C = _lgssm(2)
    ys = [np.repeat(y.numpy(), 1, axis=0) for y in model.simulate(1, 2, seed=4)]
    rng = np.random.RandomState(0)
    K = 20000
    out = contract.adapted_pass(ys, np.zeros(2), np.ones(2), None, 1.0, C, None, 0.5, [rng.randn(2, K, 2)], [])
    means, covs, _ = contract.kalman_filter(A, C, 1.0, 0.5, np.zeros(2), np.ones(2), ys)
    x = out["latents"][0]
    assert (np.abs(x.mean(axis=1) - means[0]) <= 5 * np.sqrt(np.diagonal(covs[0]) / K)).all()
    for b in range(2):
        np.testing.assert_allclose(np.cov(x[b].T), covs[0], atol=0.02)


def test_unbiased_with_a_fraction_of_the_bootstrap_variance():
    """LgssmNd(2)'s matrices, T = 5, K = 64, 512 replicas of one observation sequence: exp(log Z-hat - exact) has mean 1
    within 4 standard errors, and log Z-hat's variance is below 0.05 of a NumPy bootstrap filter's with the same K.

    Measured here (seeds as below): z-score 0.613 of the mean of exp(log Z-hat - exact) against 1; variance ratio
    0.0242 (adapted 0.00996, bootstrap 0.412).  The device test holds the same z-score bound and twice the ratio bound
    (0.1), for another random stream."""
    T, K, R = 5, 64, 512
    model, A, C = _lgssm(2)
    ys = [np.repeat(y.numpy(), R, axis=0) for y in model.simulate(T, 1, seed=1)]
    rng = np.random.RandomState(11)
    out = contract.adapted_pass(ys, np.zeros(2), np.ones(2), lambda x, t: x @ A.T, 1.0, C, None, 0.5,
                                [rng.randn(R, K, 2) for _ in range(T)], [rng.uniform(size=R) for _ in range(T - 1)])
    assert out["flags"] == 0
    _, _, exact = contract.kalman_filter(A, C, 1.0, 0.5, np.zeros(2), np.ones(2), [y[:1] for y in ys])
    log_z = out["log_marginal_likelihood"]
    ratio = np.exp(log_z - exact[0])
    z_score = abs(ratio.mean() - 1.0) / (ratio.std(ddof=1) / np.sqrt(R))
    bootstrap = contract.bootstrap_pass(ys, np.zeros(2), np.ones(2), A, 1.0, C, 0.5, K, np.random.RandomState(12))
    boot_ratio = np.exp(bootstrap - exact[0])
    assert abs(boot_ratio.mean() - 1.0) <= 4 * boot_ratio.std(ddof=1) / np.sqrt(R)      # the yardstick is itself unbiased
    variance_ratio = log_z.var(ddof=1) / bootstrap.var(ddof=1)
    print("adapted: z-score {:.3f}, var {:.3e}; bootstrap var {:.3e}; ratio {:.4f}".format(
        z_score, log_z.var(ddof=1), bootstrap.var(ddof=1), variance_ratio))
    assert z_score <= 4.0
    assert variance_ratio < 0.05
    # the last step's particle means against the exact filter
    means, covs, _ = contract.kalman_filter(A, C, 1.0, 0.5, np.zeros(2), np.ones(2), [y[:1] for y in ys])
    pooled = out["latents"][-1].mean(axis=(0, 1))
    assert (np.abs(pooled - means[-1, 0]) <= 5 * np.sqrt(np.diagonal(covs[-1]) / K)).all()


def test_kalman_filter_equals_the_models_oracle():
    from aesmc_amd.testing.models import kalman_log_likelihood
    model, A, C = _lgssm(3)
    observations = model.simulate(4, 3, seed=5)
    means, covs, total = contract.kalman_filter(A, C, 1.0, 0.5, np.zeros(3), np.ones(3), [y.numpy() for y in observations])
    np.testing.assert_allclose(total, kalman_log_likelihood(model, observations), rtol=0, atol=1e-12)
    assert means.shape == (4, 3, 3) and covs.shape == (4, 3, 3)
    single = contract.kalman_filter(A, C, 1.0, 0.5, np.zeros(3), np.ones(3), [y.numpy()[1] for y in observations])
    np.testing.assert_allclose(single[0], means[:, 1], atol=1e-14)
    assert abs(single[2] - total[1]) < 1e-12


# ---- the ABI's argument checks --------------------------------------------------------------------------------------------
def test_the_abi_rejects_bad_arguments_before_any_launch():
    """NULL pointers, negative sizes, extents below 1, an unknown dtype and a misaligned base give status 1; D or Dy above
    aesmc_affine_max_dim() or B K beyond 32-bit element arithmetic status 2; an empty problem is a no-op — no GPU needed."""
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    assert lib.aesmc_affine_max_dim() == 16
    view = _lib.View3(64, 12, 3, 1)
    ref = ctypes.byref(view)

    def quadratic(loc=ref, P=64, offset=64, out=64, B=1, K=4, D=3, Dy=2, dtype=0):
        return lib.aesmc_affine_quadratic_logweight(dtype, loc, P, offset, -1.0, out, B, K, D, Dy, None)

    assert quadratic(loc=None) == 1 and quadratic(P=None) == 1 and quadratic(offset=None) == 1 and quadratic(out=None) == 1
    assert quadratic(loc=ctypes.byref(_lib.View3(None, 12, 3, 1))) == 1
    assert quadratic(B=-1) == 1 and quadratic(K=-1) == 1 and quadratic(D=-1) == 1 and quadratic(Dy=-1) == 1
    assert quadratic(D=0) == 1 and quadratic(Dy=0) == 1 and quadratic(dtype=7) == 1
    assert quadratic(loc=ctypes.byref(_lib.View3(66, 12, 3, 1))) == 1 and quadratic(P=68) == 1 and quadratic(offset=68) == 1
    assert quadratic(out=66) == 1 and quadratic(out=68, dtype=1) == 1
    assert quadratic(D=17) == 2 and quadratic(Dy=17) == 2 and quadratic(B=1 << 16, K=1 << 16) == 2
    assert quadratic(B=0) == 0 and quadratic(K=0) == 0 and quadratic(B=0, D=17) == 0

    def draw(loc=ref, idx=64, M=64, offset=64, L=64, eps=128, out=256, flags=64, B=1, K=4, D=3, dtype=0):
        return lib.aesmc_adapted_draw(dtype, loc, idx, M, offset, L, eps, out, flags, B, K, D, None)

    assert draw(loc=None) == 1 and draw(M=None) == 1 and draw(offset=None) == 1 and draw(L=None) == 1
    assert draw(eps=None) == 1 and draw(out=None) == 1
    assert draw(loc=ctypes.byref(_lib.View3(None, 12, 3, 1))) == 1
    assert draw(B=-1) == 1 and draw(K=-1) == 1 and draw(D=-1) == 1 and draw(D=0) == 1 and draw(dtype=7) == 1
    assert draw(idx=68) == 1 and draw(M=68) == 1 and draw(L=68) == 1 and draw(offset=68) == 1 and draw(flags=66) == 1
    assert draw(eps=136) == 1 and draw(out=264) == 1 and draw(loc=ctypes.byref(_lib.View3(66, 12, 3, 1))) == 1
    assert draw(out=128) == 1 and draw(out=64) == 1                                # the output aliases an input
    assert draw(D=17) == 2 and draw(B=1 << 16, K=1 << 16) == 2
    assert draw(B=0) == 0 and draw(K=0) == 0 and draw(B=0, D=17) == 0
    assert draw(idx=None, flags=None, B=0) == 0                                    # both are optional


# ---- the host logic of adapted_filter on the oracle provider --------------------------------------------------------------
class AdaptedOracle(OracleKernels):
    """The suite's oracle provider plus the two launches from their NumPy contracts."""

    def __init__(self):
        super().__init__()
        self.calls = []

    @staticmethod
    def adapted_covers(loc, latent_dim, observation_dim):
        return torch.is_tensor(loc) and loc.dim() == 3 and loc.dtype in (torch.float32, torch.float64) and \
            loc.size(2) == latent_dim and 1 <= latent_dim <= 16 and 1 <= observation_dim <= 16

    def affine_quadratic_logweight(self, loc, P, offset, base):
        self.calls.append("quadratic")
        return torch.from_numpy(contract.affine_quadratic_logweight(loc.numpy(), P.numpy(), offset.numpy(), base))

    def adapted_draw(self, loc, index, M, offset, L, eps):
        self.calls.append("draw")
        out, flags = contract.adapted_draw(loc.numpy(), None if index is None else index.numpy(), M.numpy(), offset.numpy(),
                                           L.numpy(), eps.numpy())
        self._flags |= flags
        return torch.from_numpy(out)


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = AdaptedOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


@pytest.fixture
def counted_gains(monkeypatch):
    from aesmc_amd import adapted
    calls = []
    original = adapted.gains

    def counting(*args):
        calls.append(args)
        return original(*args)

    monkeypatch.setattr(adapted, "gains", counting)
    return calls


@pytest.mark.parametrize("family", ["affine", "plain", "nonlinear"])
def test_filter_keys_shapes_and_replay(backend, counted_gains, family):
    from aesmc_amd import adapted
    from aesmc_amd.testing.models import NonlinearSsm
    T, B, K, d = 4, 3, 9, 2
    if family == "nonlinear":
        model = NonlinearSsm(d, dtype=torch.float64)
        A, C = model.A.detach().numpy(), model.C.detach().numpy()
        location = lambda x, t: np.tanh(x @ A.T)
    else:
        model, A, C = _lgssm(d, affine=family == "affine")
        location = lambda x, t: x @ A.T
    observations = model.simulate(T, B, seed=3)
    gen = torch.Generator().manual_seed(1)
    noise = [torch.randn(B, K, d, dtype=torch.float64, generator=gen) for _ in range(T)]
    np.random.seed(5)
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, K, noise=noise,
                                 resampling="systematic", return_latents=True, return_first_stage=True)
    assert sorted(out) == ["ancestral_indices", "first_stage_log_weights", "last_latent", "latents", "log_marginal_likelihood",
                           "log_weight", "log_weights", "original_latents"]
    assert out["log_marginal_likelihood"].shape == (B,) and out["log_marginal_likelihood"].dtype == torch.float64
    assert len(out["original_latents"]) == T and all(x.shape == (B, K, d) for x in out["original_latents"])
    assert len(out["log_weights"]) == T and all(w.shape == (B, K) and not w.any() for w in out["log_weights"])
    assert out["log_weight"] is out["log_weights"][-1] and out["last_latent"] is out["original_latents"][-1]
    assert len(out["ancestral_indices"]) == T - 1
    assert all(a.shape == (B, K) and a.dtype == torch.int64 for a in out["ancestral_indices"])
    assert len(out["first_stage_log_weights"]) == T - 1 and all(w.shape == (B, K) for w in out["first_stage_log_weights"])
    assert len(out["latents"]) == T and torch.equal(out["latents"][-1], out["original_latents"][-1])
    assert backend.calls == ["draw"] + ["quadratic", "draw"] * (T - 1)
    # one computation for step 0 (the initial's scale) and ONE for all later steps of a time-invariant model
    assert len(counted_gains) == 2
    # the same numbers as the restated filter fed the same noise and uniforms
    np.random.seed(5)
    uniforms = [np.random.uniform(size=[B, 1]).reshape(-1) for _ in range(T - 1)]
    want = contract.adapted_pass([y.numpy() for y in observations], np.zeros(d), np.ones(d), location, 1.0, C, None, 0.5,
                                 [e.numpy() for e in noise], uniforms)
    assert min(want["margins"]) > 1e-9
    for got, expected in zip(out["ancestral_indices"], want["ancestral_indices"]):
        assert np.array_equal(got.numpy(), expected)
    for got, expected, tolerance in zip(out["original_latents"], want["latents"], want["tolerances"]["latents"]):
        assert np.abs(got.numpy() - expected).max() <= tolerance
    assert np.abs(out["log_marginal_likelihood"].numpy() - want["log_marginal_likelihood"]).max() <= \
        want["tolerances"]["log_marginal_likelihood"]
    # replay: the same noise and uniforms give the same run; without return_* the optional entries are None
    np.random.seed(5)
    again = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, K, noise=noise)
    assert again["latents"] is None and again["first_stage_log_weights"] is None
    assert all(torch.equal(a, b) for a, b in zip(again["original_latents"], out["original_latents"]))
    assert torch.equal(again["log_marginal_likelihood"], out["log_marginal_likelihood"])


def test_one_step_filter_is_exact_on_the_host_path(backend):
    from aesmc_amd import adapted
    from aesmc_amd.testing.models import kalman_log_likelihood
    model, _, _ = _lgssm(3, affine=True)
    observations = model.simulate(1, 4, seed=8)
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, 5)
    np.testing.assert_allclose(out["log_marginal_likelihood"].numpy(), kalman_log_likelihood(model, observations),
                               rtol=0, atol=1e-10)
    assert out["ancestral_indices"] == [] and backend.calls == ["draw"]


def test_gain_cache_pays_per_step_for_a_time_varying_emission(backend, counted_gains):
    from aesmc_amd import adapted
    from aesmc_amd.linear_gaussian import AffineNormal
    T, B, K, d = 5, 2, 6, 2
    model, _, _ = _lgssm(d, affine=True)
    weights = [model.C.detach() * (1.0 + 0.1 * t) for t in range(T)]
    offsets = [None, torch.ones(d, dtype=torch.float64), torch.ones(B, d, dtype=torch.float64), None, None]

    def emission(latents=None, time=None, previous_observations=None):
        return model._tag(AffineNormal(latents[-1], weights[time], model.emission_scale, offset=offsets[time]),
                          "FULLY_EXPANDED")

    out = adapted.adapted_filter(model.simulate(T, B, seed=3), model.initial, model.transition, emission, K)
    assert len(counted_gains) == T and torch.isfinite(out["log_marginal_likelihood"]).all()


def test_refusals_come_before_the_steps_launches(backend):
    from aesmc_amd import adapted
    from aesmc_amd.linear_gaussian import AffineNormal
    from aesmc_amd.testing.models import LearnedScaleSsm
    model, _, _ = _lgssm(2, affine=True)
    observations = model.simulate(3, 2, seed=3)
    run = lambda **kw: adapted.adapted_filter(
        kw.pop("observations", observations), kw.pop("initial", model.initial), kw.pop("transition", model.transition),
        kw.pop("emission", model.emission), 4, **kw)

    def refused(text, **kw):
        backend.calls.clear()
        with pytest.raises(NotImplementedError, match="covered: ") as caught:
            run(**kw)
        assert text in str(caught.value)
        return list(backend.calls)

    assert refused("dict", observations=[{"y": y} for y in observations]) == []
    assert refused("dict", initial=lambda: {"x": model.initial()}) == []
    assert refused("type", initial=lambda: torch.distributions.Laplace(model.loc0, model.scale0)) == []
    assert refused("shape", initial=lambda: torch.distributions.Normal(torch.zeros(2, 3, 2), 1.0)) == []
    assert refused("D > 16", initial=lambda: torch.distributions.Normal(torch.zeros(17, dtype=torch.float64), 1.0)) == []
    assert refused("dtype", initial=lambda: torch.distributions.Normal(torch.zeros(2, dtype=torch.float16), 1.0)) == []
    batch_scale = torch.rand(2, 2, dtype=torch.float64) + 0.5
    assert refused("varies", initial=lambda: torch.distributions.Normal(torch.zeros(2, 2, dtype=torch.float64),
                                                                        batch_scale)) == []
    # an emission that is not linear in the newest latent: refused before step 0's draw
    curved = lambda latents=None, time=None, previous_observations=None: model._tag(
        torch.distributions.Normal(torch.tanh(latents[-1]), model.emission_scale), "FULLY_EXPANDED")
    assert refused("not linear-Gaussian", emission=curved) == []
    elsewhere = lambda latents=None, time=None, previous_observations=None: model._tag(
        AffineNormal(latents[-1] * 1.0, model.C, model.emission_scale), "FULLY_EXPANDED")
    assert refused("other than latents[-1]", emission=elsewhere) == []
    wide = torch.zeros(17, 2, dtype=torch.float64)
    tall = lambda latents=None, time=None, previous_observations=None: model._tag(
        AffineNormal(latents[-1], wide, model.emission_scale), "FULLY_EXPANDED")
    assert refused("observations of shape", emission=tall) == []
    assert refused("Dy > 16", emission=tall, observations=[torch.zeros(2, 17, dtype=torch.float64)] * 3) == []
    # a transition `_normal_terms` refuses: after step 0, before step 1's launches
    varying = LearnedScaleSsm(2, dtype=torch.float64)
    laplace = lambda previous_latents=None, time=None, previous_observations=None: model._tag(
        torch.distributions.Laplace(previous_latents[-1], model.transition_scale), "FULLY_EXPANDED")
    assert refused("Laplace", transition=laplace) == ["draw"]
    per_particle = lambda previous_latents=None, time=None, previous_observations=None: model._tag(
        torch.distributions.Normal(previous_latents[-1], previous_latents[-1].abs() + 1.0), "FULLY_EXPANDED")
    assert refused("particle-dependent", transition=per_particle) == ["draw"]
    assert varying.transition is not None
    # arguments
    with pytest.raises(ValueError, match="resampling"):
        run(resampling="multinomial")
    with pytest.raises(ValueError, match="noise"):
        run(noise=[torch.zeros(2, 4, 2, dtype=torch.float64)])
    with pytest.raises(ValueError, match="noise\\[0\\]"):
        run(noise=[torch.zeros(2, 4, 2)] * 3)
    with pytest.raises(ValueError, match="num_particles"):
        adapted.adapted_filter(observations, model.initial, model.transition, model.emission, 0)


def test_a_flagged_run_raises_at_the_end_and_the_next_starts_clean(backend):
    from aesmc_amd import adapted
    model, _, _ = _lgssm(2, affine=True)
    observations = model.simulate(3, 2, seed=3)
    poisoned = lambda previous_latents=None, time=None, previous_observations=None: model._tag(
        torch.distributions.Normal(previous_latents[-1] * float("nan"), model.transition_scale, validate_args=False),
        "FULLY_EXPANDED")
    with pytest.raises(FloatingPointError):
        adapted.adapted_filter(observations, model.initial, poisoned, model.emission, 4)
    out = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, 4)
    assert torch.isfinite(out["log_marginal_likelihood"]).all()


def test_the_output_feeds_the_smoothers_contract_unchanged(backend):
    """`original_latents` and `log_weights` have the shapes and dtypes `smoothing.backward_simulate` documents."""
    from aesmc_amd import adapted
    model, _, _ = _lgssm(2, affine=True)
    out = adapted.adapted_filter(model.simulate(3, 2, seed=3), model.initial, model.transition, model.emission, 4)
    for x, w in zip(out["original_latents"], out["log_weights"]):
        assert x.shape[:2] == w.shape and x.dtype == w.dtype == torch.float64
