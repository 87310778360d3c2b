"""CPU checks of the differentiable adapted filter: the NumPy contracts of K29 / K30 (aesmc_amd/testing/adapted.py)
against torch.autograd of the plain formulas within their derived bounds, the ABI's argument checks of the three new
entries, and `aesmc_amd.adapted.adapted_elbo` — on the suite's oracle provider with the four launches attached from their
contracts — against `adapted_elbo_restated` (value and every gradient), against `adapted_filter` (the same forward
numbers), for what it asks of the provider, and, at T = 2, against the gradient of the Kalman filter's log-likelihood."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as contract
from tests import gradient_checks as checks
from tests.test_adapted_contract import AdaptedOracle


# ---- the two contracts against autograd -------------------------------------------------------------------------------------
def _leaf(array):
    return torch.from_numpy(np.ascontiguousarray(array)).double().requires_grad_(True)


@pytest.mark.parametrize("B,K,D,Dy", [(3, 7, 4, 3), (2, 5, 1, 1), (1, 33, 10, 16)])
def test_quadratic_backward_contract_against_autograd(B, K, D, Dy):
    rng = np.random.RandomState(K)
    loc, P, o, g = rng.randn(B, K, D), rng.randn(Dy, D), rng.randn(B, Dy), rng.randn(B, K)
    tl, tP, to = _leaf(loc), _leaf(P), _leaf(o)
    value = -1.5 - 0.5 * ((tl @ tP.t() + to.unsqueeze(1)) ** 2).sum(dim=2)
    want = torch.autograd.grad((value * torch.from_numpy(g)).sum(), [tl, tP, to])
    got = contract.affine_quadratic_logweight_backward(loc, P, o, g)
    bounds = contract.affine_quadratic_logweight_backward_bound(loc, P, o, g)
    for name, mine, reference, bound in zip(("loc", "P", "offset"), got, want, bounds):
        assert mine.shape == tuple(reference.shape) == bound.shape, name
        assert (np.abs(mine - reference.numpy()) <= bound).all(), name
        assert bound.max() < 1e-11, name
    # a particle stride of zero; float32 operands: grad_loc is rounded once, the sums stay float64
    row = np.broadcast_to(loc[:, :1].astype(np.float32), (B, K, D))
    single = contract.affine_quadratic_logweight_backward(row, P, o, g.astype(np.float32))
    assert single[0].dtype == np.float32 and single[1].dtype == np.float64 and single[2].dtype == np.float64
    wide = contract.affine_quadratic_logweight_backward(row.astype(np.float64), P, o, g.astype(np.float32))
    assert np.array_equal(single[0], wide[0].astype(np.float32)) and np.array_equal(single[1], wide[1])


@pytest.mark.parametrize("index", ["none", "sorted", "one"])
@pytest.mark.parametrize("B,K,D", [(3, 7, 4), (2, 5, 1), (1, 33, 10)])
def test_draw_backward_contract_against_autograd(B, K, D, index):
    rng = np.random.RandomState(K)
    loc, eps, G = rng.randn(B, K, D), rng.randn(B, K, D), rng.randn(B, K, D)
    M, L, r = rng.randn(D, D), np.tril(rng.randn(D, D)), rng.randn(B, D)
    idx = {"none": None, "sorted": np.sort(rng.randint(0, K, size=(B, K)), axis=1), "one": np.full((B, K), K // 2)}[index]
    tl, tM, tL, tr = _leaf(loc), _leaf(M), _leaf(L), _leaf(r)
    moved = tl if idx is None else checks.gather_rows(tl, torch.from_numpy(idx))
    x = tr.unsqueeze(1) + moved @ tM.t() + torch.from_numpy(eps) @ torch.tril(tL).t()
    grad_moved, = torch.autograd.grad((x * torch.from_numpy(G)).sum(), [moved], retain_graph=True)
    want = (grad_moved,) + torch.autograd.grad((x * torch.from_numpy(G)).sum(), [tM, tL, tr])
    junk = L + np.triu(np.full((D, D), np.nan), 1)                       # L's values are not read
    got = contract.adapted_draw_backward(loc, idx, M, junk, eps, G)
    bounds = contract.adapted_draw_backward_bound(loc, idx, M, junk, eps, G)
    assert got[4] == 0
    for name, mine, reference, bound in zip(("h", "M", "L", "r"), got, want, bounds):
        assert mine.shape == tuple(reference.shape) == bound.shape, name
        assert (np.abs(mine - reference.numpy()) <= bound).all(), name
        assert bound.max() < 1e-11, name
    assert not np.triu(got[2], 1).any() and not np.triu(bounds[2], 1).any()


def test_draw_backward_contract_out_of_range():
    rng = np.random.RandomState(1)
    B, K, D = 3, 7, 4
    loc, eps, G, M = rng.randn(B, K, D), rng.randn(B, K, D), rng.randn(B, K, D), rng.randn(D, D)
    idx = rng.randint(0, K, size=(B, K))
    bad = idx.copy()
    bad[1, 2], bad[2, 0] = K, -1
    clean = contract.adapted_draw_backward(loc, idx, M, M, eps, G)
    h, grad_M, grad_L, grad_r, flags = contract.adapted_draw_backward(loc, bad, M, M, eps, G)
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE
    hit = bad != idx
    assert np.isnan(h[hit]).all() and np.array_equal(h[~hit], clean[0][~hit])
    silenced = np.where(hit[:, :, None], 0.0, G)                          # the particle contributes nothing
    want = contract.adapted_draw_backward(loc, idx, M, M, eps, silenced)
    assert np.array_equal(grad_M, want[1]) and np.array_equal(grad_L, want[2]) and np.array_equal(grad_r, want[3])
    assert not contract.adapted_draw_backward_bound(loc, bad, M, M, eps, G)[0][hit].any()


# ---- the ABI's argument checks --------------------------------------------------------------------------------------------
def test_the_abi_rejects_bad_arguments_before_any_launch():
    """NULL or misaligned pointers, no output at all, an output that aliases an input, negative sizes, extents below 1, an
    unknown dtype and a workspace that is missing or too small give status 1; D or Dy above 16 or B K beyond 32-bit element
    arithmetic status 2; an empty problem is a no-op — no GPU needed."""
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    size = lib.aesmc_adapted_backward_workspace_bytes
    assert size(1, 4, 3, 2) > 0 and size(1, 4, 3, 2) % 8 == 0 and size(4, 4096, 10, 10) >= size(1, 4, 3, 2)
    assert size(1024, 4096, 10, 10) <= 64 << 20                          # a fixed block plus 4 bytes per particle
    assert size(0, 4, 3, 2) == 0 and size(1, 4, 17, 2) == 0 and size(1, 4, 3, 17) == 0 and size(1 << 16, 1 << 16, 3, 2) == 0
    enough = size(1, 4, 3, 2)
    view = _lib.View3(64, 12, 3, 1)
    ref = ctypes.byref(view)

    def quadratic(loc=ref, P=64, offset=64, grad=64, grad_loc=256, grad_P=512, grad_offset=1024, ws=2048, ws_bytes=enough,
                  B=1, K=4, D=3, Dy=2, dtype=0):
        return lib.aesmc_affine_quadratic_logweight_backward(dtype, loc, P, offset, grad, grad_loc, grad_P, grad_offset, ws,
                                                             ws_bytes, B, K, D, Dy, None)

    assert quadratic(loc=None) == 1 and quadratic(P=None) == 1 and quadratic(offset=None) == 1 and quadratic(grad=None) == 1
    assert quadratic(loc=ctypes.byref(_lib.View3(None, 12, 3, 1))) == 1
    assert quadratic(grad_loc=None, grad_P=None, grad_offset=None) == 1                 # nothing to compute
    assert quadratic(B=-1) == 1 and quadratic(K=-1) == 1 and quadratic(D=-1) == 1 and quadratic(Dy=-1) == 1
    assert quadratic(D=0) == 1 and quadratic(Dy=0) == 1 and quadratic(dtype=7) == 1
    assert quadratic(loc=ctypes.byref(_lib.View3(66, 12, 3, 1))) == 1 and quadratic(P=68) == 1 and quadratic(offset=68) == 1
    assert quadratic(grad=66) == 1 and quadratic(grad=68, dtype=1) == 1 and quadratic(grad_loc=264) == 1
    assert quadratic(grad_P=516) == 1 and quadratic(grad_offset=1028) == 1 and quadratic(ws=2052) == 1
    assert quadratic(grad_loc=64) == 1 and quadratic(grad_P=64) == 1 and quadratic(grad_offset=64) == 1   # aliases
    assert quadratic(ws=None) == 1 and quadratic(ws_bytes=enough - 8) == 1 and quadratic(ws_bytes=-1) == 1
    assert quadratic(D=17) == 2 and quadratic(Dy=17) == 2 and quadratic(B=1 << 16, K=1 << 16) == 2
    assert quadratic(B=0) == 0 and quadratic(K=0) == 0 and quadratic(B=0, D=17) == 0
    assert quadratic(B=0, grad_P=None, grad_offset=None, ws=None, ws_bytes=0) == 0      # the outputs are optional

    def draw(loc=ref, idx=64, M=64, eps=128, grad=192, h=256, grad_M=512, grad_L=1024, grad_r=1536, flags=64, ws=2048,
             ws_bytes=enough, B=1, K=4, D=3, dtype=0):
        return lib.aesmc_adapted_draw_backward(dtype, loc, idx, M, eps, grad, h, grad_M, grad_L, grad_r, flags, ws, ws_bytes,
                                               B, K, D, None)

    assert draw(loc=None) == 1 and draw(M=None) == 1 and draw(eps=None) == 1 and draw(grad=None) == 1
    assert draw(loc=ctypes.byref(_lib.View3(None, 12, 3, 1))) == 1
    assert draw(h=None, grad_M=None, grad_L=None, grad_r=None) == 1                     # nothing to compute
    assert draw(B=-1) == 1 and draw(K=-1) == 1 and draw(D=-1) == 1 and draw(D=0) == 1 and draw(dtype=7) == 1
    assert draw(idx=68) == 1 and draw(M=68) == 1 and draw(flags=66) == 1 and draw(eps=136) == 1 and draw(grad=200) == 1
    assert draw(h=264) == 1 and draw(grad_M=516) == 1 and draw(grad_L=1028) == 1 and draw(grad_r=1540) == 1
    assert draw(ws=2052) == 1 and draw(loc=ctypes.byref(_lib.View3(66, 12, 3, 1))) == 1
    assert draw(h=128) == 1 and draw(h=192) == 1 and draw(h=64) == 1 and draw(grad_M=64) == 1 and draw(grad_L=64) == 1
    assert draw(grad_L=512) == 1                                                        # two outputs in one place
    assert draw(ws=None) == 1 and draw(ws_bytes=enough - 8) == 1 and draw(ws_bytes=-1) == 1
    assert draw(D=17) == 2 and draw(B=1 << 16, K=1 << 16) == 2
    assert draw(B=0) == 0 and draw(K=0) == 0 and draw(B=0, D=17) == 0
    assert draw(idx=None, flags=None, grad_M=None, grad_L=None, grad_r=None, ws=None, ws_bytes=0, B=0) == 0
    assert lib.aesmc_version() == 501


# ---- adapted_elbo on the oracle provider ------------------------------------------------------------------------------------
class DifferentiableOracle(AdaptedOracle):
    """The suite's oracle provider plus all four launches of a differentiable adapted step from their NumPy contracts."""

    def __init__(self):
        super().__init__()
        self.asked = []

    def affine_quadratic_logweight_backward(self, loc, P, offset, grad, need_loc=True, need_P=True, need_offset=True):
        self.calls.append("quadratic_backward")
        self.asked.append(("quadratic", need_loc, need_P, need_offset))
        out = contract.affine_quadratic_logweight_backward(loc.numpy(), P.numpy(), offset.numpy(), grad.numpy())
        return tuple(torch.from_numpy(np.ascontiguousarray(t)) if wanted else None
                     for t, wanted in zip(out, (need_loc, need_P, need_offset)))

    def adapted_draw_backward(self, loc, index, M, L, eps, grad, need_h=True, need_M=True, need_L=True, need_r=True):
        self.calls.append("draw_backward")
        self.asked.append(("draw", need_h, need_M, need_L, need_r))
        out = contract.adapted_draw_backward(loc.numpy(), None if index is None else index.numpy(), M.numpy(), L.numpy(),
                                             eps.numpy(), grad.numpy())
        self._flags |= out[4]
        return tuple(torch.from_numpy(np.ascontiguousarray(t)) if wanted else None
                     for t, wanted in zip(out[:4], (need_h, need_M, need_L, need_r)))


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = DifferentiableOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


LEAVES = ("A", "C", "loc0", "scale0", "transition_scale", "emission_scale")


def _model(family, dim, dtype=torch.float64, device="cpu"):
    """(model, its leaves by name, the transition's location as a torch function of them)."""
    from aesmc_amd.testing.models import LgssmNd, NonlinearSsm
    if family == "nonlinear":
        model = NonlinearSsm(dim, dtype=dtype).to(device)
        location = lambda x, t: torch.tanh(x @ model.A.to(x.dtype).t())
    else:
        model = LgssmNd(dim, dtype=dtype, affine=family == "affine").to(device)
        location = lambda x, t: x @ model.A.to(x.dtype).t()
    leaves = {name: getattr(model, name) for name in LEAVES}
    for leaf in leaves.values():
        leaf.requires_grad_(True)
    return model, leaves, location


def _restated(model, location, observations, noise, ancestors, dtype=None):
    return contract.adapted_elbo_restated(observations, model.loc0, model.scale0, location, model.transition_scale, model.C,
                                          None, model.emission_scale, noise, ancestors, dtype=dtype)


def _gradients(value, leaves):
    grads = torch.autograd.grad(value.sum(), list(leaves.values()), allow_unused=True)
    return {name: grad for name, grad in zip(leaves, grads)}


def compare_with_restatement(out, model, leaves, location, observations, noise, limit=checks.FLOAT64_TOLERANCE):
    """The value and every leaf's gradient of a run against the float64 restatement fed the run's own ancestors and noise,
    under tests/gradient_checks.py's reduced metric (max|got - want| / max|want|, no floor).  Returns the errors."""
    want = _restated(model, location, [y.double() for y in observations], [e.double() for e in noise],
                     out["ancestral_indices"])
    errors = {"value": checks.reduced_error(out["log_marginal_likelihood"].detach(),
                                            want["log_marginal_likelihood"].detach())}
    got_grads = _gradients(out["log_marginal_likelihood"], leaves)
    want_grads = _gradients(want["log_marginal_likelihood"], leaves)
    for name in leaves:
        assert got_grads[name] is not None and want_grads[name] is not None, name
        errors[name] = checks.reduced_error(got_grads[name], want_grads[name])
    assert max(errors.values()) <= limit, errors
    return errors


@pytest.mark.parametrize("family", ["affine", "plain", "nonlinear"])
def test_elbo_equals_the_restatement_and_the_filter(backend, family):
    from aesmc_amd import adapted
    T, B, K, d = 4, 3, 9, 2
    model, leaves, location = _model(family, d)
    observations = model.simulate(T, B, seed=3)
    gen = torch.Generator().manual_seed(1)
    noise = [torch.randn(B, K, d, dtype=torch.float64, generator=gen) for _ in range(T)]
    np.random.seed(5)
    out = adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, K, noise=noise,
                               resampling="systematic")
    assert sorted(out) == ["ancestral_indices", "last_latent", "log_marginal_likelihood", "log_weight", "log_weights",
                           "original_latents"]
    assert out["log_marginal_likelihood"].shape == (B,) and out["log_marginal_likelihood"].dtype == torch.float64
    assert out["log_marginal_likelihood"].requires_grad
    assert backend.calls == ["draw"] + ["quadratic", "draw"] * (T - 1)
    compare_with_restatement(out, model, leaves, location, observations, noise)
    assert "draw_backward" in backend.calls and "quadratic_backward" in backend.calls
    # the forward numbers are the filter's
    np.random.seed(5)
    with torch.no_grad():
        same = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, K, noise=noise,
                                      resampling="systematic")
    assert torch.equal(same["log_marginal_likelihood"], out["log_marginal_likelihood"].detach())
    assert all(torch.equal(a, b.detach()) for a, b in zip(same["original_latents"], out["original_latents"]))
    assert all(torch.equal(a, b) for a, b in zip(same["ancestral_indices"], out["ancestral_indices"]))
    assert all(not w.any() and not w.requires_grad for w in out["log_weights"])


def test_loss_is_minus_the_batch_mean(backend):
    from aesmc_amd import adapted
    model, leaves, _ = _model("affine", 2)
    observations = model.simulate(3, 4, seed=2)
    gen = torch.Generator().manual_seed(4)
    noise = [torch.randn(4, 5, 2, dtype=torch.float64, generator=gen) for _ in range(3)]
    np.random.seed(2)
    out = adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, 5, noise=noise)
    np.random.seed(2)
    loss = adapted.adapted_loss(observations, model.initial, model.transition, model.emission, 5, noise=noise)
    assert loss.dim() == 0 and torch.equal(loss, -out["log_marginal_likelihood"].mean())
    loss.backward()
    assert torch.isfinite(model.A.grad).all() and model.A.grad.abs().max() > 0
    assert model.C.grad is not None and model.Wx.grad is None          # there is no proposal to learn


def test_only_what_needs_a_gradient_is_asked_for(backend):
    """T = 2 with only C requiring grad: step 0's draw has a location nobody differentiates (the initial's), so its
    backward is not asked for h; step 1's first-stage weights see x_0 — a function of C through M, r and L — so theirs
    is asked for the location's gradient and for P's; step 1's draw reaches nothing and has no backward at all."""
    from aesmc_amd import adapted
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(2, dtype=torch.float64, affine=False)
    for parameter in model.parameters():
        parameter.requires_grad_(False)
    model.C.requires_grad_(True)
    observations = model.simulate(2, 3, seed=3)
    out = adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, 6)
    out["log_marginal_likelihood"].sum().backward()
    assert backend.asked == [("quadratic", True, True, True), ("draw", False, True, True, True)]
    assert model.C.grad is not None and model.A.grad is None


def test_refusals_and_scopes(backend):
    from aesmc_amd import adapted, distributed
    model, _, _ = _model("affine", 2)
    observations = model.simulate(3, 2, seed=3)
    with pytest.raises(NotImplementedError, match="shard_scope"):
        with distributed.shard_scope(4, 0, 2):
            adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, 4)
    curved = lambda latents=None, time=None, previous_observations=None: model._tag(
        torch.distributions.Normal(torch.tanh(latents[-1]), model.emission_scale), "FULLY_EXPANDED")
    with pytest.raises(NotImplementedError, match="covered: "):
        adapted.adapted_elbo(observations, model.initial, model.transition, curved, 4)
    with pytest.raises(ValueError, match="noise"):
        adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, 4,
                             noise=[torch.zeros(2, 4, 2, dtype=torch.float64)])
    with pytest.raises(ValueError, match="num_particles"):
        adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, 0)
    # under torch.no_grad() the caller still gets a graph: the filter enables autograd itself
    with torch.no_grad():
        out = adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, 4)
    assert out["log_marginal_likelihood"].requires_grad


# ---- T = 2: no resampling lies on the gradient's path ---------------------------------------------------------------------
def _kalman_log_likelihood(A, C, s_f, s_g, loc0, scale0, ys):
    """`testing.adapted.kalman_filter`'s log-likelihood [B], restated in torch (float64, differentiable)."""
    Dy, D = C.shape
    B = ys[0].shape[0]
    Q, R = torch.eye(D, dtype=torch.float64) * s_f ** 2, torch.eye(Dy, dtype=torch.float64) * s_g ** 2
    mean, cov = loc0.expand(B, D), torch.diag(scale0 ** 2)
    total = torch.zeros(B, dtype=torch.float64)
    for t, y in enumerate(ys):
        if t > 0:
            mean, cov = mean @ A.t(), A @ cov @ A.t() + Q
        S = C @ cov @ C.t() + R
        residual = y - mean @ C.t()
        solved = torch.linalg.solve(S, residual.t()).t()
        total = total - 0.5 * ((residual * solved).sum(dim=1) + torch.linalg.slogdet(S)[1] + Dy * np.log(2 * np.pi))
        gain = cov @ C.t() @ torch.linalg.inv(S)
        mean, cov = mean + residual @ gain.t(), cov - gain @ C @ cov
    return total


@pytest.mark.parametrize("which", ["restated", "elbo"])
def test_gradient_at_two_steps_is_the_kalman_gradient(backend, which):
    """LgssmNd(2), T = 2, B = 4, K = 4096, 16 seeds: the seed-mean of the gradient of sum_b log Z-hat with respect to A and
    C against the autograd gradient of the Kalman filter's log-likelihood, elementwise within five standard errors of
    that seed-mean.  `restated`: the pure-torch restatement alone holds the assertion (with ancestors that its one
    resampling step never lets reach a gradient), so what `elbo` is held to is the estimator's, not the code's."""
    from aesmc_amd import adapted
    T, B, K, d, seeds = 2, 4, 4096, 2, 16
    model, leaves, location = _model("plain", d)
    observations = model.simulate(T, B, seed=7)
    grads = {"A": [], "C": []}
    for seed in range(seeds):
        gen = torch.Generator().manual_seed(100 + seed)
        noise = [torch.randn(B, K, d, dtype=torch.float64, generator=gen) for _ in range(T)]
        if which == "elbo":
            np.random.seed(seed)
            value = adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, K,
                                         noise=noise)["log_marginal_likelihood"]
        else:
            ancestors = [torch.arange(K).expand(B, K).contiguous()]
            value = _restated(model, location, observations, noise, ancestors)["log_marginal_likelihood"]
        got = torch.autograd.grad(value.sum(), [model.A, model.C])
        grads["A"].append(got[0]), grads["C"].append(got[1])
    exact = _kalman_log_likelihood(model.A, model.C, model.transition_scale, model.emission_scale, model.loc0, model.scale0,
                                   observations)
    host = lambda t: t.detach().numpy()
    _, _, numpy_total = contract.kalman_filter(host(model.A), host(model.C), host(model.transition_scale),
                                               host(model.emission_scale), host(model.loc0), host(model.scale0),
                                               [host(y) for y in observations])
    np.testing.assert_allclose(host(exact), numpy_total, rtol=0, atol=1e-10)
    want = dict(zip(("A", "C"), torch.autograd.grad(exact.sum(), [model.A, model.C])))
    for name in ("A", "C"):
        stack = torch.stack(grads[name])
        mean, error = stack.mean(dim=0), stack.std(dim=0, unbiased=True) / np.sqrt(seeds)
        z = ((mean - want[name]).abs() / error).max()
        print("{} d/d{}: largest z-score {:.3f}, standard errors up to {:.2e} of gradients up to {:.2e}".format(
            which, name, float(z), float(error.max()), float(want[name].abs().max())))
        assert ((mean - want[name]).abs() <= 5.0 * error).all(), (name, mean, want[name], error)
