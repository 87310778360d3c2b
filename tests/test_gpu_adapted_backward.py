"""The differentiable adapted filter on the device: kernels K29 (aesmc_affine_quadratic_logweight_backward) and K30
(aesmc_adapted_draw_backward) against their NumPy contracts (aesmc_amd/testing/adapted.py) within the contracts' derived
bounds — every layout of the location, every kind of index, batch rows inside a wavefront's 64 particles, across
wavefronts, across tiles and across workgroups —, their determinism and out-of-range convention, and
`aesmc_amd.adapted.adapted_elbo` end to end against the pure-torch restatement, in float64 and in float32, and through an
optimiser step."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import adapted as contract
from tests import gradient_checks as checks

pytestmark = pytest.mark.gpu

# (2,300,3,2): a tile spans two rows, a partial tile, several workgroups; (3,8,10,10): K27 / K28's 33-row offset table;
# (5,3,1,1): no offset table, rows inside a wavefront's chunk; (1,513,16,16): a row over three tiles at full width
SHAPES = [(2, 300, 3, 2), (3, 8, 10, 10), (5, 3, 1, 1), (1, 513, 16, 16), (2, 256, 4, 7)]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _device_loc(loc, layout, device):
    """(`loc` on the device, what it holds on the host): dense, its first particle read with particle stride 0 ('row'),
    or a view whose three strides are (K D, 1, K) ('strided': nothing of it is contiguous)."""
    t = torch.from_numpy(loc).to(device)
    if layout == "row":
        return t[:, :1].contiguous().expand(loc.shape), np.broadcast_to(loc[:, :1], loc.shape)
    if layout == "strided":
        view = t.transpose(1, 2).contiguous().transpose(1, 2)
        assert not view.is_contiguous() or loc.shape[1] == 1 or loc.shape[2] == 1
        return view, loc
    return t, loc


def _inside(got, want, bound):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound


def _assert_inside(name, got, want, bound):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, name
    ok = _inside(got, want, bound)
    assert ok.all(), (name, np.argwhere(~ok)[:4], np.abs(got.astype(np.float64) - want).max(), bound.max())


@pytest.mark.parametrize("layout", ["dense", "row", "strided"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D,Dy", SHAPES)
def test_quadratic_backward_equals_contract(hip_device, B, K, D, Dy, dtype, layout):
    provider = _provider()
    rng = np.random.RandomState(7 * K + D)
    loc = (2.0 * rng.randn(B, K, D)).astype(dtype)
    P, o, g = np.eye(Dy, D) + 0.3 * rng.randn(Dy, D), rng.randn(B, Dy), rng.randn(B, K).astype(dtype)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    device_loc, host_loc = _device_loc(loc, layout, hip_device)
    got = provider.affine_quadratic_logweight_backward(device_loc, dev(P), dev(o), dev(g))
    want = contract.affine_quadratic_logweight_backward(host_loc, P, o, g)
    bounds = contract.affine_quadratic_logweight_backward_bound(host_loc, P, o, g)
    assert got[0].dtype == TORCH[dtype] and got[0].is_contiguous() and got[1].dtype == got[2].dtype == torch.float64
    for name, mine, reference, bound in zip(("grad_loc", "grad_P", "grad_offset"), got, want, bounds):
        _assert_inside(name, mine, reference, bound)
    # only what is asked for is returned, and it is the same
    only = provider.affine_quadratic_logweight_backward(device_loc, dev(P), dev(o), dev(g), need_loc=False, need_P=False)
    assert only[0] is None and only[1] is None and torch.equal(only[2], got[2])
    assert provider.read_flags(hip_device) == 0


def _index(kind, B, K, rng):
    if kind == "none":
        return None
    if kind == "one":
        return np.full((B, K), K // 3, dtype=np.int64)
    return np.sort(rng.randint(0, K, size=(B, K)), axis=1).astype(np.int64)      # (with repeats and gaps)


@pytest.mark.parametrize("layout", ["dense", "row", "strided"])
@pytest.mark.parametrize("index", ["none", "sorted", "one"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D,Dy", SHAPES)
def test_draw_backward_equals_contract(hip_device, B, K, D, Dy, dtype, index, layout):
    provider = _provider()
    rng = np.random.RandomState(11 * K + D)
    loc, eps, G = [(s * rng.randn(B, K, D)).astype(dtype) for s in (2.0, 1.0, 1.0)]
    M = np.eye(D) + 0.3 * rng.randn(D, D)
    idx = _index(index, B, K, rng)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    device_loc, host_loc = _device_loc(loc, layout, hip_device)
    unread = dev(np.full((D, D), np.nan))                                   # L is taken for its shape only
    got = provider.adapted_draw_backward(device_loc, dev(idx), dev(M), unread, dev(eps), dev(G))
    want = contract.adapted_draw_backward(host_loc, idx, M, np.zeros((D, D)), eps, G)
    bounds = contract.adapted_draw_backward_bound(host_loc, idx, M, np.zeros((D, D)), eps, G)
    assert want[4] == 0 and got[0].dtype == TORCH[dtype] and got[0].is_contiguous()
    for name, mine, reference, bound in zip(("h", "grad_M", "grad_L", "grad_r"), got, want, bounds):
        _assert_inside(name, mine, reference, bound)
    assert not torch.triu(got[2], 1).any()                                  # exactly zero above the diagonal
    only = provider.adapted_draw_backward(device_loc, dev(idx), dev(M), unread, dev(eps), dev(G), need_h=False, need_M=False,
                                          need_r=False)
    assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2], got[2])
    assert provider.read_flags(hip_device) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D,Dy", [(2, 300, 3, 2), (1, 513, 16, 16), (40, 3500, 10, 10)])
def test_two_identical_calls_return_the_same_bits(hip_device, B, K, D, Dy, dtype):
    """(40, 3500, 10, 10): 547 tiles for 512 workgroups — some walk two —, rows that start inside a wavefront's chunk."""
    provider = _provider()
    rng = np.random.RandomState(3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    loc, eps, G = [dev(rng.randn(B, K, D).astype(dtype)) for _ in range(3)]
    P, o, g, M = dev(rng.randn(Dy, D)), dev(rng.randn(B, Dy)), dev(rng.randn(B, K).astype(dtype)), dev(rng.randn(D, D))
    idx = dev(np.sort(rng.randint(0, K, size=(B, K)), axis=1))
    first = provider.affine_quadratic_logweight_backward(loc, P, o, g) + provider.adapted_draw_backward(loc, idx, M, M, eps, G)
    junk = torch.full((1 << 22,), float("nan"), dtype=torch.float64, device=hip_device)     # (what a freed workspace may hold)
    del junk
    again = provider.affine_quadratic_logweight_backward(loc, P, o, g) + provider.adapted_draw_backward(loc, idx, M, M, eps, G)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(torch.isfinite(t).all() for t in first)
    # and the results are the contracts' at this size too
    host = lambda t: t.cpu().numpy()
    want = contract.affine_quadratic_logweight_backward(host(loc), host(P), host(o), host(g))
    bounds = contract.affine_quadratic_logweight_backward_bound(host(loc), host(P), host(o), host(g))
    for name, mine, reference, bound in zip(("grad_loc", "grad_P", "grad_offset"), first[:3], want, bounds):
        _assert_inside(name, mine, reference, bound)
    want = contract.adapted_draw_backward(loc.cpu().numpy(), idx.cpu().numpy(), M.cpu().numpy(), M.cpu().numpy(),
                                          eps.cpu().numpy(), G.cpu().numpy())
    bounds = contract.adapted_draw_backward_bound(loc.cpu().numpy(), idx.cpu().numpy(), M.cpu().numpy(), M.cpu().numpy(),
                                                  eps.cpu().numpy(), G.cpu().numpy())
    for name, mine, reference, bound in zip(("h", "grad_M", "grad_L", "grad_r"), first[3:], want, bounds):
        _assert_inside(name, mine, reference, bound)
    assert provider.read_flags(hip_device) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_index_out_of_range_gives_nan_rows_and_the_flag(hip_device, dtype):
    from aesmc_amd import _lib
    provider = _provider()
    B, K, D = 3, 300, 10
    rng = np.random.RandomState(5)
    loc, eps, G = [rng.randn(B, K, D).astype(dtype) for _ in range(3)]
    M = rng.randn(D, D)
    idx = np.sort(rng.randint(0, K, size=(B, K)), axis=1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    clean = provider.adapted_draw_backward(dev(loc), dev(idx), dev(M), dev(M), dev(eps), dev(G))
    assert provider.read_flags(hip_device) == 0
    bad = idx.copy()
    bad[0, 0], bad[1, 299], bad[2, 256] = K, -1, 1 << 40
    got = provider.adapted_draw_backward(dev(loc), dev(bad), dev(M), dev(M), dev(eps), dev(G))
    assert provider.read_flags(hip_device) == _lib.FLAG_INDEX_OUT_OF_RANGE
    hit = torch.from_numpy(bad != idx).to(hip_device)
    assert torch.isnan(got[0][hit]).all() and torch.equal(got[0][~hit], clean[0][~hit])
    want = contract.adapted_draw_backward(loc, bad, M, M, eps, G)
    bounds = contract.adapted_draw_backward_bound(loc, bad, M, M, eps, G)
    assert want[4] == contract.FLAG_INDEX_OUT_OF_RANGE
    for name, mine, reference, bound in zip(("grad_M", "grad_L", "grad_r"), got[1:], want[1:4], bounds[1:]):
        _assert_inside(name, mine, reference, bound)                      # the three particles contribute nothing
    again = provider.adapted_draw_backward(dev(loc), dev(idx), dev(M), dev(M), dev(eps), dev(G))
    assert provider.read_flags(hip_device) == 0 and all(torch.equal(a, b) for a, b in zip(again, clean))


def test_provider_refuses_what_the_kernels_do_not_take(hip_device):
    provider = _provider()
    loc = torch.zeros(2, 4, 3, device=hip_device)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=hip_device)
    with pytest.raises(ValueError, match="P must be"):
        provider.affine_quadratic_logweight_backward(loc, f64(2, 4), f64(2, 2), torch.zeros(2, 4, device=hip_device))
    with pytest.raises(ValueError, match="gradient must be"):
        provider.affine_quadratic_logweight_backward(loc, f64(2, 3), f64(2, 2), f64(2, 4))
    with pytest.raises(ValueError, match="M must be"):
        provider.adapted_draw_backward(loc, None, f64(3, 2), f64(3, 3), torch.zeros_like(loc), torch.zeros_like(loc))
    with pytest.raises(ValueError, match="gradient must be"):
        provider.adapted_draw_backward(loc, None, f64(3, 3), f64(3, 3), torch.zeros_like(loc), f64(2, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        provider.adapted_draw_backward(loc.cpu(), None, f64(3, 3), f64(3, 3), torch.zeros_like(loc), torch.zeros_like(loc))
    empty = provider.adapted_draw_backward(loc[:0], None, f64(3, 3), f64(3, 3), torch.zeros_like(loc[:0]),
                                           torch.zeros_like(loc[:0]))
    assert tuple(empty[0].shape) == (0, 4, 3) and not empty[1].any() and tuple(empty[3].shape) == (0, 3)


# ---- the whole differentiable filter ----------------------------------------------------------------------------------------
class _Ssm(torch.nn.Module):
    """x_0 ~ N(loc0, diag(scale0^2)), x_t ~ N(f(A x_{t-1}), diag(s_f^2)), y_t ~ N(C x_t + offset, diag(s_g^2)) with f the
    identity ('lgssm') or tanh ('nonlinear'), Dy != D, per-dimension scales: every leaf the filter differentiates."""

    def __init__(self, family, dim, dim_y, dtype, seed=0):
        super().__init__()
        from aesmc_amd import state
        self._state, self.family, self.dim, self.dim_y = state, family, dim, dim_y
        rng = np.random.RandomState(seed)
        leaf = lambda a: torch.nn.Parameter(torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype))
        self.A = leaf(0.8 * np.eye(dim) + 0.1 * rng.randn(dim, dim))
        self.C = leaf(np.eye(dim_y, dim) + 0.2 * rng.randn(dim_y, dim))
        self.offset = leaf(0.3 * rng.randn(dim_y))
        self.loc0 = leaf(0.2 * rng.randn(dim))
        self.scale0 = leaf(1.0 + 0.2 * rng.rand(dim))
        self.transition_scale = leaf(0.7 + 0.3 * rng.rand(dim))
        self.emission_scale = leaf(0.4 + 0.2 * rng.rand(dim_y))

    def _tag(self, dist, mode_name):
        return self._state.set_batch_shape_mode(dist, getattr(self._state.BatchShapeMode, mode_name))

    def location(self, x, t=None):
        loc = x @ self.A.to(x.dtype).t()
        return torch.tanh(loc) if self.family == "nonlinear" else loc

    def initial(self):
        return self._tag(torch.distributions.Normal(self.loc0, self.scale0, validate_args=False), "NOT_EXPANDED")

    def transition(self, previous_latents=None, time=None, previous_observations=None):
        return self._tag(torch.distributions.Normal(self.location(previous_latents[-1]), self.transition_scale,
                                                    validate_args=False), "FULLY_EXPANDED")

    def emission(self, latents=None, time=None, previous_observations=None):
        from aesmc_amd.linear_gaussian import AffineNormal
        return self._tag(AffineNormal(latents[-1], self.C, self.emission_scale, offset=self.offset, validate_args=False),
                         "FULLY_EXPANDED")

    @torch.no_grad()
    def simulate(self, num_timesteps, batch_size, seed=0):
        gen = torch.Generator().manual_seed(seed)
        device, dtype = self.A.device, self.A.dtype
        noise = lambda size: torch.randn(batch_size, size, generator=gen, dtype=torch.float64).to(device, dtype)
        x = self.loc0 + self.scale0 * noise(self.dim)
        observations = []
        for time in range(num_timesteps):
            if time > 0:
                x = self.location(x) + self.transition_scale * noise(self.dim)
            observations.append(x @ self.C.t() + self.offset + self.emission_scale * noise(self.dim_y))
        return observations

    def leaves(self):
        return dict(self.named_parameters())


def _restated(model, observations, noise, ancestors, dtype):
    return contract.adapted_elbo_restated(observations, model.loc0, model.scale0, model.location, model.transition_scale,
                                          model.C, model.offset, model.emission_scale, noise, ancestors, dtype=dtype)


def _value_and_gradients(value, leaves):
    grads = torch.autograd.grad(value.sum(), list(leaves.values()), allow_unused=True)
    assert all(grad is not None for grad in grads), [name for name, grad in zip(leaves, grads) if grad is None]
    return dict(zip(leaves, grads), value=value.detach())


def _errors(got, want):
    """tests/gradient_checks.py's reduced metric (max|got - want| / max|want|) of the value and of every leaf's gradient,
    both as `_value_and_gradients` returns them."""
    return {name: checks.reduced_error(got[name], want[name]) for name in want}


def _run(model, K, T, B, resampling, seed):
    from aesmc_amd import adapted
    observations = model.simulate(T, B, seed=2)
    gen = torch.Generator().manual_seed(seed)
    noise = [torch.randn(B, K, model.dim, generator=gen, dtype=torch.float64).to(model.A.device, model.A.dtype)
             for _ in range(T)]
    np.random.seed(seed)
    torch.manual_seed(seed)
    out = adapted.adapted_elbo(observations, model.initial, model.transition, model.emission, K, resampling=resampling,
                               noise=noise)
    return observations, noise, out


@pytest.mark.parametrize("resampling", ["systematic", "stratified"])
@pytest.mark.parametrize("family", ["lgssm", "nonlinear"])
def test_whole_run_in_float64_against_the_restatement(hip_device, family, resampling):
    T, B, K, d, Dy = 4, 3, 300, 3, 2
    model = _Ssm(family, d, Dy, torch.float64).to(hip_device)
    observations, noise, out = _run(model, K, T, B, resampling, seed=9)
    assert out["log_marginal_likelihood"].dtype == torch.float64 and out["log_marginal_likelihood"].requires_grad
    assert all(a.dtype == torch.int64 and bool((a[:, 1:] >= a[:, :-1]).all()) for a in out["ancestral_indices"])
    want = _restated(model, observations, noise, out["ancestral_indices"], torch.float64)
    for got, expected in zip(out["original_latents"], want["latents"]):
        assert float((got.detach() - expected.detach()).abs().max()) <= 1e-9
    leaves = model.leaves()
    errors = _errors(_value_and_gradients(out["log_marginal_likelihood"], leaves),
                     _value_and_gradients(want["log_marginal_likelihood"], leaves))
    print("float64 {} {}: {}".format(family, resampling, {k: "{:.2e}".format(v) for k, v in errors.items()}))
    assert max(errors.values()) <= checks.FLOAT64_TOLERANCE, errors
    assert _provider().read_flags(hip_device) == 0


@pytest.mark.parametrize("resampling", ["systematic", "stratified"])
@pytest.mark.parametrize("family", ["lgssm", "nonlinear"])
def test_whole_run_in_float32_against_the_float64_restatement(hip_device, family, resampling):
    """The float32 run against the float64 restatement fed its ancestors and its noise, upcast; the allowance for the
    value and for every gradient is twice the error the pure-torch FLOAT32 restatement shows against the float64 one on
    the same inputs.  The kernels accumulate in float64 and the gains are formed in float64; the errors measured on an
    MI355X are in profiles/adapted_backward.txt."""
    T, B, K, d, Dy = 4, 3, 300, 3, 2
    model = _Ssm(family, d, Dy, torch.float32).to(hip_device)
    observations, noise, out = _run(model, K, T, B, resampling, seed=9)
    assert out["log_marginal_likelihood"].dtype == torch.float64 and out["last_latent"].dtype == torch.float32
    ancestors = out["ancestral_indices"]
    # the reference differentiates a float64 copy of the model: its gradients are not rounded to the float32 leaves
    wide = _Ssm(family, d, Dy, torch.float64).to(hip_device)
    with torch.no_grad():
        for target, source in zip(wide.parameters(), model.parameters()):
            target.copy_(source)
    want = _restated(wide, [y.double() for y in observations], [e.double() for e in noise], ancestors,
                     torch.float64)["log_marginal_likelihood"]
    single = _restated(model, observations, noise, ancestors, torch.float32)["log_marginal_likelihood"]
    leaves = model.leaves()
    exact = _value_and_gradients(want, wide.leaves())
    mine = _errors(_value_and_gradients(out["log_marginal_likelihood"], leaves), exact)
    reference = _errors(_value_and_gradients(single, leaves), exact)
    for name in mine:
        print("float32 {} {} {:>16}: run {:.2e}, float32 restatement {:.2e}".format(family, resampling, name, mine[name],
                                                                                   reference[name]))
    for name in mine:
        assert mine[name] <= 2.0 * reference[name], (name, mine[name], reference[name])
    assert _provider().read_flags(hip_device) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_an_optimiser_step_through_adapted_loss(hip_device, dtype):
    from aesmc_amd import adapted
    model = _Ssm("lgssm", 3, 2, dtype).to(hip_device)
    observations = model.simulate(5, 4, seed=1)
    before = {name: p.detach().clone() for name, p in model.named_parameters()}
    optimiser = torch.optim.SGD(model.parameters(), lr=1e-3)
    torch.manual_seed(0)
    np.random.seed(0)
    loss = adapted.adapted_loss(observations, model.initial, model.transition, model.emission, 257)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and torch.isfinite(loss)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.dtype == dtype for p in model.parameters())
    optimiser.step()
    assert all(not torch.equal(p.detach(), before[name]) for name, p in model.named_parameters())
    assert _provider().read_flags(hip_device) == 0
