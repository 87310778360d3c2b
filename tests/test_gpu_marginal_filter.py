"""The marginal particle filter on the device: kernel K25 (aesmc_pairwise_pass) against its NumPy contract
(aesmc_amd/testing/marginal_filter.py) within the contract's own bound, its views, its conventions for special values, the
autograd operator `_ops.pairwise_lse` over K22 and K25, and `infer("mpf")` / `get_loss(algorithm="vmpf")` end to end:
against the contract's recursion on the run's own particles, against a plain PyTorch CPU float64 restatement with explicit
[K,K] matrices for the gradients, the proposal == transition identity, and unbiasedness against the Kalman filter."""
import math

import numpy as np
import pytest
import torch
from torch import nn
from torch.distributions import Normal

from aesmc_amd.testing import marginal_filter as contract
from aesmc_amd.testing import smoothing as lse_contract
from tests.test_gpu_marginal_smoothing import _held, _operands as _lse_operands

pytestmark = pytest.mark.gpu

# (B, N, M, D): N below, at and off the tile of 4 (2) own points; M below, at and above a wavefront's 64 others and 256; D
# = 0, 1, the maximum, and no multiple of 4; above and below the 16 dimensions of one chunk
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 1), (3, 5, 7, 2), (2, 64, 64, 3), (2, 33, 65, 10), (3, 100, 257, 1), (2, 17, 1000, 10),
          (2, 40, 300, 17), (1, 16, 128, 128), (1, 4, 50, 256), (1, 9, 4097, 2), (3, 5, 7, 0)]
PROFILES = ("flat", "wide", "minus_inf_stretch", "tied", "dominant", "far", "shifted")


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _forward_operands(profile, B, R, C, D, dtype, seed, one_scale=False):
    """K22's operands for one profile, its stored result in `dtype`, and a gradient arriving at it.  "shifted": both
    clouds moved by 1000 scales — where an accumulation of raw moments would lose everything."""
    rows, cols, scale, col_a, col_sub, row_add = _lse_operands("unit" if profile == "shifted" else profile, B, R, C, D,
                                                               dtype, seed)
    if profile == "shifted":
        rows, cols = (rows + 1000 * scale).astype(dtype), (cols + 1000 * scale).astype(dtype)
    if one_scale:
        scale = scale[:1]      # one value for the whole point
    out = lse_contract.pairwise_lse(rows, cols, scale, col_a, col_sub, row_add)[0].astype(dtype)
    grad = np.random.RandomState(seed + 1).randn(B, R).astype(dtype)
    return rows, cols, scale, col_a, col_sub, row_add, out, grad


def _sides(rows, cols, scale, col_a, col_sub, row_add, out, grad):
    """The two passes of K22's backward as `pairwise_pass` operands of the operands' dtype."""
    dtype = out.dtype
    L, term, absent_or_minus_l = contract._backward_terms(col_a, col_sub, row_add, out)
    cast = lambda a: a.astype(dtype)
    return (dict(own=rows, others=cols, scale=scale, own_term=cast(-L), other_term=cast(term), own_gain=grad, other_gain=None),
            dict(own=cols, others=rows, scale=scale, own_term=cast(term), other_term=cast(absent_or_minus_l), own_gain=None,
                 other_gain=grad))


def _launch(device, want_mass=True, want_pull=True, want_spread=True, **operands):
    """The kernel on NumPy operands -> (mass, pull, spread, flags) as NumPy."""
    provider = _provider()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert provider.read_flags(device) == 0
    out = provider.pairwise_pass(**{name: dev(value) for name, value in operands.items()}, want_mass=want_mass,
                                 want_pull=want_pull, want_spread=want_spread)
    flags = provider.read_flags(device)
    return tuple(None if t is None else t.cpu().numpy() for t in out) + (flags,)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,N,M,D", SHAPES)
def test_kernel_equals_contract_within_its_bound(hip_device, dtype, B, N, M, D):
    rng = np.random.RandomState(N + M)
    for number, profile in enumerate(PROFILES):
        if D == 0 and profile in ("tied", "far", "shifted"):
            continue      # (no distance term: nothing to tie or to move)
        forward = _forward_operands(profile, B, N, M, max(D, 1), dtype, 100 * number + M % 89, one_scale=number % 2 == 1)
        if D == 0:      # (the stored result of the D == 0 forward: formed without the distance term)
            tail = forward[3:6]
            out = lse_contract.pairwise_lse(np.zeros((B, N, 0)), np.zeros((B, M, 0)), None, *tail)[0].astype(dtype)
            forward = (forward[0][:, :, :0], forward[1][:, :, :0], None) + tail + (out, forward[7])
        for side, operands in enumerate(_sides(*forward)):
            # with both gains (one of them the side's own), with that one alone, and — every other profile — with none
            extra = rng.randn(*operands["own_term" if side else "other_term"].shape).astype(dtype)
            variants = [dict(operands), dict(operands, **{("own_gain" if side else "other_gain"): extra})]
            if number % 2:
                variants.append(dict(operands, own_gain=None, other_gain=None))
            for which, variant in enumerate(variants):
                want = contract.pairwise_pass(**variant)
                bounds = contract.pairwise_pass_bound(**variant)
                # every nullable output present, and one launch that leaves one of them out
                wanted = [(True, True, True)]
                if which == 0:
                    wanted.append([(False, True, True), (True, False, True), (True, True, False), (False, True, False)]
                                  [(number + side) % 4])
                for flags_wanted in wanted:
                    got = _launch(hip_device, *flags_wanted, **variant)
                    assert want[3] == 0 and got[3] == 0, (profile, side, got[3])
                    for name, value, reference, bound, asked in zip(("mass", "pull", "spread"), got, want, bounds,
                                                                    flags_wanted):
                        if not asked:
                            assert value is None
                            continue
                        assert value.dtype == dtype
                        if name == "mass" or D:
                            _held(value, reference, bound, (profile, side, which, flags_wanted, name))
                        else:
                            assert value.shape == reference.shape and value.shape[2] == 0


def test_views_give_what_dense_copies_give(hip_device):
    provider = _provider()
    B, N, M, D = 3, 21, 300, 5
    gen = torch.Generator(device=hip_device).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=hip_device, generator=gen)
    own_term, other_term, own_gain, other_gain = -3 + rand(B, N), rand(B, M) - 3, rand(B, N), rand(B, M)
    others_mb = rand(M, B, D)                      # stored [M,B,D]
    own_big = rand(B, N + 7, 2 * D + 1)
    scale = 0.5 + torch.rand(D, device=hip_device, generator=gen)
    others, own = others_mb.transpose(0, 1), own_big[:, 3:3 + N, 1::2]
    assert not others.is_contiguous() and not own.is_contiguous()
    for s in (scale, scale[:1], scale[0]):
        dense = provider.pairwise_pass(own.contiguous(), others.contiguous(), s.clone(), own_term, other_term, own_gain,
                                       other_gain)
        views = provider.pairwise_pass(own, others, s, own_term, other_term, own_gain, other_gain)
        assert all(torch.equal(a, b) for a, b in zip(dense, views))
        assert views[0].shape == (B, N) and views[1].shape == views[2].shape == (B, N, D)
        want = contract.pairwise_pass(own.cpu().numpy(), others.cpu().numpy(), s.reshape(-1).cpu().numpy(),
                                      own_term.cpu().numpy(), other_term.cpu().numpy(), own_gain.cpu().numpy(),
                                      other_gain.cpu().numpy())
        for a, b in zip(views, want[:3]):
            assert np.abs(a.cpu().numpy() - b).max() < 1e-4 * (1 + np.abs(b).max())
    wide_term = rand(B, 2 * M) - 3
    assert all(torch.equal(a, b) for a, b in zip(
        provider.pairwise_pass(own, others, scale, own_term, wide_term[:, ::2]),
        provider.pairwise_pass(own, others, scale, own_term, wide_term[:, ::2].contiguous())))
    # a [B,N] tensor is D = 1; a [B,N,2,3] one is D = 6
    flat = provider.pairwise_pass(own[..., 0], others[..., 0], scale[:1], own_term, other_term)
    again = provider.pairwise_pass(own[..., :1], others[..., :1], scale[:1], own_term, other_term)
    assert all(torch.equal(a, b) for a, b in zip(flat, again)) and flat[1].shape == (B, N, 1)
    own6, others6 = rand(B, N, 2, 3), rand(B, M, 2, 3)
    assert all(torch.equal(a, b) for a, b in zip(
        provider.pairwise_pass(own6, others6, scale[:1], own_term, other_term),
        provider.pairwise_pass(own6.reshape(B, N, 6), others6.reshape(B, M, 6), scale[:1], own_term, other_term)))
    assert provider.read_flags(hip_device) == 0
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_pass(own, others, scale, own_term.double(), other_term)
    with pytest.raises(ValueError, match="does not take these operands"):
        provider.pairwise_pass(own, others[:, :-1], scale, own_term, other_term)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        provider.pairwise_pass(own.cpu(), others.cpu(), scale.cpu(), own_term.cpu(), other_term.cpu())


def test_a_bad_own_point_flags_and_leaves_the_others_alone(hip_device):
    B, N, M, D = 4, 21, 300, 3
    forward = _forward_operands("unit", B, N, M, D, np.float32, 5)
    base = _sides(*forward)[0]
    base["other_gain"] = np.random.RandomState(2).randn(B, M).astype(np.float32)
    clean = _launch(hip_device, **base)
    assert clean[3] == 0 and all(np.isfinite(v).all() for v in clean[:3])

    def check(affected, bit, value, **changed):
        operands = dict(base)
        for name, (index, v) in changed.items():
            operands[name] = operands[name].copy()
            operands[name][index] = v
        want = contract.pairwise_pass(**operands)
        got = _launch(hip_device, **operands)
        assert got[3] == bit == want[3], (changed, got[3], want[3])
        for out, reference, untouched in zip(got[:3], want[:3], clean[:3]):
            assert np.array_equal(out[affected], np.full(out[affected].shape, value, dtype=np.float32), equal_nan=True), changed
            assert np.array_equal(np.isnan(out), np.isnan(reference))
            assert np.array_equal(out[~affected].view(np.uint32), untouched[~affected].view(np.uint32)), changed
        assert _provider().read_flags(hip_device) == 0          # the status word is clear afterwards

    everything = np.ones((B, N), dtype=bool)
    row = lambda b: everything & (np.arange(B) == b)[:, None]
    one = np.zeros((B, N), dtype=bool)
    one[0, 13] = True
    nan_flag = contract.FLAG_NAN_LOG_WEIGHT
    check(row(1), nan_flag, np.nan, other_term=((1, 70), np.nan))
    check(row(1), nan_flag, np.nan, other_term=((1, 70), np.inf))
    check(row(2), nan_flag, np.nan, others=((2, 299, 1), np.nan))
    check(row(2), nan_flag, np.nan, other_gain=((2, 257), np.nan))
    check(one, nan_flag, np.nan, own=((0, 13, 2), np.nan))            # one own point of one batch row
    check(one, nan_flag, np.nan, own_gain=((0, 13), np.nan))
    check(everything, nan_flag, np.nan, scale=(1, np.nan))
    for term in (-np.inf, np.inf, np.nan):                            # not a finite own term: zeros, no flag
        check(one, 0, 0.0, own_term=((0, 13), term), own=((0, 13, 0), np.nan), own_gain=((0, 13), np.nan))
    # an absent other stays absent whatever it holds: nothing is flagged, nothing is NaN, the other batch rows keep their bits
    for poison in (np.nan, np.inf):
        operands = {name: None if value is None else value.copy() for name, value in base.items()}
        operands["other_term"][1, 40] = -np.inf
        operands["others"][1, 40] = poison
        operands["other_gain"][1, 40] = poison
        got, want, bounds = _launch(hip_device, **operands), contract.pairwise_pass(**operands), \
            contract.pairwise_pass_bound(**operands)
        assert got[3] == 0
        for out, reference, bound, untouched in zip(got[:3], want[:3], bounds, clean[:3]):
            _held(out, reference, bound, poison)
            assert np.array_equal(np.delete(out, 1, 0), np.delete(untouched, 1, 0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,R,C,D", [(2, 33, 65, 10), (2, 64, 64, 3)])
def test_the_operator_is_k22_forwards_and_the_contracts_assembly_backwards(hip_device, dtype, B, R, C, D):
    from aesmc_amd import _ops
    provider = _provider()
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    rows, cols, scale, col_a, col_sub, row_add = _lse_operands("unit", B, R, C, D, np_dtype, 11)
    col_a[1, 5] = -np.inf      # an absent column
    grad = np.random.RandomState(12).randn(B, R).astype(np_dtype)
    for scale_np in (scale, scale[:1]):
        numpy_operands = (rows, cols, scale_np, col_a, col_sub, row_add)
        leaves = [torch.from_numpy(a).to(hip_device).requires_grad_(True) for a in numpy_operands]
        out = _ops.pairwise_lse(*leaves)
        stored = provider.pairwise_lse(*[t.detach() for t in leaves])
        assert torch.equal(out.detach(), stored) and out.dtype == dtype
        got = torch.autograd.grad(out, leaves, torch.from_numpy(grad).to(hip_device))
        assert provider.read_flags(hip_device) == 0
        stored_np = stored.cpu().numpy()
        want, flags = contract.pairwise_lse_backward(*numpy_operands, stored_np, grad)
        bounds = contract.pairwise_lse_backward_bound(*numpy_operands, stored_np, grad)
        assert flags == 0
        for name, value, leaf in zip(("rows", "cols", "scale", "col_a", "col_sub", "row_add"), got, leaves):
            assert value.shape == leaf.shape and value.dtype == dtype
            _held(value.cpu().numpy(), want[name].reshape(value.shape), bounds[name].reshape(value.shape), name)
        assert float(got[3][1, 5]) == 0.0 and float(got[4][1, 5]) == 0.0 and bool((got[1][1, 5] == 0).all())


# ---- through the API ------------------------------------------------------------------------------------------------------
class Forms(nn.Module):
    """x_0 ~ N(0, I), x_t ~ N(loc_f(x_{t-1}), s_f^2), y_t ~ N(C x_t, s_g^2), proposal N(loc_q(x_{t-1}) + Wy y_t, s_q^2) with
    per-dimension scales that are parameters, in the three forms the smoothing tests use."""

    def __init__(self, form, d, dtype):
        super().__init__()
        gen = torch.Generator().manual_seed(d)
        eye = torch.eye(d, dtype=torch.float64)
        noisy = lambda base: nn.Parameter((base * eye + 0.05 * torch.randn(d, d, generator=gen, dtype=torch.float64)).to(dtype))
        self.form, self.d = form, d
        self.A, self.C, self.Wx, self.Wy, self.W0 = noisy(0.9), noisy(1.0), noisy(0.45), noisy(0.5), noisy(0.5)
        self.offset = nn.Parameter(torch.linspace(-0.2, 0.2, d, dtype=torch.float64).to(dtype))
        self.s_f = nn.Parameter(torch.linspace(0.9, 1.2, d, dtype=torch.float64).to(dtype))
        self.s_q = nn.Parameter(torch.linspace(0.8, 0.6, d, dtype=torch.float64).to(dtype))
        self.register_buffer("s_g", torch.tensor(0.5, dtype=dtype))
        self.register_buffer("zero", torch.zeros(d, dtype=dtype))
        self.register_buffer("one", torch.ones(d, dtype=dtype))

    @staticmethod
    def _tag(dist, name):
        from aesmc_amd import state
        return state.set_batch_shape_mode(dist, getattr(state.BatchShapeMode, name))

    def locations(self, x, y):
        """(loc_f, loc_q) of the stored particles x [B,K,d] for the next step's observation y [B,d]: plain arithmetic."""
        if self.form == "tanh":
            return torch.tanh(x @ self.A.t()), torch.tanh(x @ self.Wx.t()) + (y @ self.Wy.t()).unsqueeze(1)
        return x @ self.A.t() + self.offset, x @ self.Wx.t() + (y @ self.Wy.t()).unsqueeze(1)

    def initial(self):
        return self._tag(Normal(self.zero, self.one), "NOT_EXPANDED")

    def transition(self, previous_latents=None, time=None, previous_observations=None):
        from aesmc_amd.linear_gaussian import AffineNormal
        assert len(previous_latents) == time and all(type(x) is torch.Tensor for x in previous_latents)
        x = previous_latents[-1]
        if self.form == "affine_normal":
            return self._tag(AffineNormal(x, self.A, self.s_f, offset=self.offset), "FULLY_EXPANDED")
        return self._tag(Normal(self.locations(x, x[:, 0])[0], self.s_f), "FULLY_EXPANDED")

    def emission(self, latents=None, time=None, previous_observations=None):
        return self._tag(Normal(latents[-1] @ self.C.t(), self.s_g), "FULLY_EXPANDED")

    def proposal(self, previous_latents=None, time=None, observations=None):
        from aesmc_amd.linear_gaussian import AffineNormal
        if time == 0:
            return self._tag(Normal(observations[0] @ self.W0.t(), self.s_q), "BATCH_EXPANDED")
        x = previous_latents[-1]
        if self.form == "affine_normal":
            return self._tag(AffineNormal(x, self.Wx, self.s_q, offset=observations[time] @ self.Wy.t()), "FULLY_EXPANDED")
        return self._tag(Normal(self.locations(x, observations[time])[1], self.s_q), "FULLY_EXPANDED")


def _restated_loss(model, observations, stored, indices):
    """-mean log Z of the marginal particle filter in plain PyTorch float64 on the CPU with explicit [K,K] matrices, on
    the run's own ancestor indices and its own noise, recovered from the stored particles as eps = (x_t - loc_q[idx]) /
    s_q; a copy of the model holds the leaves.  Returns (loss, named gradients)."""
    twin = Forms(model.form, model.d, torch.float64)
    twin.load_state_dict({name: value.detach().cpu().double() for name, value in model.state_dict().items()})
    y = [o.detach().cpu().double() for o in observations]
    x_stored = [x.detach().cpu().double() for x in stored]
    indices = [i.cpu() for i in indices]
    d, K = model.d, x_stored[0].shape[1]

    def normal(value, loc, s):
        return (-0.5 * ((value - loc) / s) ** 2 - torch.log(s) - 0.5 * math.log(2 * math.pi)).sum(-1)

    def mixture(value, loc, s, log_w):
        q = (((value[:, :, None, :] - loc[:, None, :, :]) / s) ** 2).sum(-1)
        return torch.logsumexp(log_w[:, None, :] - 0.5 * q, dim=2) - torch.log(s).sum()

    loc = (y[0] @ twin.W0.t()).unsqueeze(1)
    with torch.no_grad():
        eps = (x_stored[0] - loc) / twin.s_q
    x = loc + twin.s_q * eps
    log_w = normal(x, twin.zero, twin.one) + normal(y[0].unsqueeze(1), x @ twin.C.t(), twin.s_g.expand(d)) - \
        normal(x, loc, twin.s_q)
    log_z = torch.logsumexp(log_w, 1) - math.log(K)
    for t in range(1, len(y)):
        loc_f, loc_q = twin.locations(x, y[t])
        chosen = torch.gather(loc_q, 1, indices[t - 1][:, :, None].expand(-1, -1, d))
        with torch.no_grad():
            eps = (x_stored[t] - chosen) / twin.s_q
        x = chosen + twin.s_q * eps
        log_g = normal(y[t].unsqueeze(1), x @ twin.C.t(), twin.s_g.expand(d))
        log_w = log_g + (mixture(x, loc_f, twin.s_f, log_w) - mixture(x, loc_q, twin.s_q, log_w))
        log_z = log_z + torch.logsumexp(log_w, 1) - math.log(K)
    loss = -log_z.mean()
    used = {name: p for name, p in twin.named_parameters() if not (twin.form == "tanh" and name == "offset")}
    return loss.detach(), dict(zip(used, torch.autograd.grad(loss, list(used.values()))))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("K,d", [(33, 2), (130, 3)])
@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul", "tanh"])
def test_infer_mpf_and_the_vmpf_loss(hip_device, form, K, d, dtype):
    from aesmc_amd import inference, losses
    from aesmc_amd.testing import replay
    B, T = 3, 4
    model = Forms(form, d, dtype).to(hip_device)
    gen = torch.Generator().manual_seed(7)
    observations = [torch.randn(B, d, generator=gen, dtype=torch.float64).to(hip_device, dtype) for _ in range(T)]
    torch.manual_seed(3)
    np.random.seed(3)
    with replay.record() as tape:
        out = inference.infer("mpf", observations, model.initial, model.transition, model.emission, model.proposal, K,
                              return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                              return_log_weights=True, return_ancestral_indices=True)
    stored, indices = out["original_latents"], out["ancestral_indices"]
    assert len(tape.normals) == T and len(tape.uniforms) == T - 1
    assert all(x.shape == (B, K, d) and x.dtype == dtype for x in stored) and all(i.shape == (B, K) for i in indices)
    # the returned log-weights and log Z against the contract's recursion on the run's own stored particles
    with torch.no_grad():
        pairs = {t: model.locations(stored[t - 1], observations[t]) for t in range(1, T)}
        if form == "affine_normal":      # (K8's chain, as the run formed them)
            pairs = {t: (model.transition(previous_latents=stored[:t], time=t).loc,
                         model.proposal(previous_latents=stored[:t], time=t, observations=observations).loc)
                     for t in range(1, T)}
        log_g = [Normal(x @ model.C.t(), model.s_g).log_prob(y.unsqueeze(1)).sum(-1).cpu().numpy()
                 for x, y in zip(stored, observations)]
    n = lambda t: t.detach().cpu().numpy()
    want_w, want_z, (tolerance, z_tolerance) = contract.marginal_filter_pass(
        [n(x) for x in stored], [n(i) for i in indices], lambda t: n(pairs[t][1]), lambda t: n(pairs[t][0]), n(model.s_q),
        n(model.s_f), log_g, n(out["log_weights"][0]), return_tolerance=True)
    for t in range(T):
        error = np.abs(n(out["log_weights"][t]).astype(np.float64) - want_w[t].astype(np.float64))
        assert (error <= tolerance[t]).all(), (t, error.max(), tolerance[t].min())
    error = np.abs(n(out["log_marginal_likelihood"]).astype(np.float64) - want_z.astype(np.float64))
    assert (error <= z_tolerance).all(), (error, z_tolerance)
    # the loss and its parameter gradients, on the same draws, against the CPU float64 restatement on the same indices
    with replay.replay(tape):
        loss = losses.get_loss(observations, K, "vmpf", model.initial, model.transition, model.emission, model.proposal)
    want_loss, want = _restated_loss(model, observations, stored, indices)
    parameters = {name: p for name, p in model.named_parameters() if name in want}      # (the tanh form has no offset)
    got = dict(zip(parameters, torch.autograd.grad(loss, list(parameters.values()))))
    assert len(want) >= 7
    f64 = dtype == torch.float64
    assert abs(float(loss.detach()) - float(want_loss)) <= (1e-10 if f64 else 1e-4) * (1 + abs(float(want_loss)))
    for name, wanted in want.items():
        scale = float(wanted.abs().max()) + 1e-30
        assert scale > 1e-6, name
        np.testing.assert_allclose(got[name].detach().cpu().double().numpy() / scale, wanted.numpy() / scale, rtol=0,
                                   atol=1e-8 if f64 else 1e-3, err_msg=name)


def test_a_proposal_that_is_the_transition_gives_the_emission_alone(hip_device):
    from aesmc_amd import inference, state
    from aesmc_amd.testing.models import LgssmNd
    T, B, K = 4, 3, 130
    model = LgssmNd(3).to(hip_device)
    observations = model.simulate(T, B, seed=1)

    def proposal(previous_latents=None, time=None, observations=None):
        if time == 0:
            return model.proposal(time=0, observations=observations)
        return model.transition(previous_latents=previous_latents, time=time)

    torch.manual_seed(3)
    np.random.seed(3)
    with torch.no_grad():
        out = inference.infer("mpf", observations, model.initial, model.transition, model.emission, proposal, K,
                              return_original_latents=True, return_log_weights=True, return_latents=False)
        for t in range(1, T):
            log_g = state.log_prob(model.emission(latents=out["original_latents"][:t + 1], time=t),
                                   state.expand_observation(observations[t], K))
            assert torch.equal(out["log_weights"][t], log_g)


def test_the_estimate_is_unbiased_against_the_kalman_filter(hip_device):
    """test_gpu_infer.py::test_smc_estimate_is_unbiased_against_kalman_filter's model and data, 1024 runs as a batch, K =
    256: |log mean exp(log Z - exact)| < 0.05, that test's bound.  A CPU float64 simulation of the algorithm over six
    seeds stayed within 0.0083 at this shape (standard deviation of log Z per run 0.19, of the batch mean 0.006)."""
    from aesmc_amd import inference
    from aesmc_amd.testing import models
    torch.manual_seed(0)
    np.random.seed(0)
    model = models.LgssmNd(2, seed=0, dtype=torch.float64, validate_args=False).to(hip_device)
    observations = model.simulate(5, 1, seed=2)
    exact = float(models.kalman_log_likelihood(model, observations)[0])
    repeated = [o.expand(1024, -1).contiguous() for o in observations]
    with torch.no_grad():
        out = inference.infer("mpf", repeated, model.initial, model.transition, model.emission, model.proposal, 256,
                              return_log_marginal_likelihood=True, return_latents=False)
    estimates = out["log_marginal_likelihood"].cpu().numpy()
    error = np.log(np.mean(np.exp(estimates - exact)))
    print("\n[marginal particle filter] log mean exp(log Z - exact) = {:.4f}, sd of log Z {:.3f}".format(error, estimates.std()))
    assert abs(error) < 0.05, (error, exact)
