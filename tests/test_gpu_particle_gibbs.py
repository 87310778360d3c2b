"""Particle Gibbs with ancestor sampling on the device: kernel K26 (aesmc_conditional_ancestor_index) against its NumPy
contract (aesmc_amd/testing/particle_gibbs.py) — indices and flags — and against K21 on the device, its views, its
conventions for bad rows, an independent frequency check, and `aesmc_amd.particle_gibbs` end to end: against the NumPy
sweep on the contract model and against the exact (Rauch-Tung-Striebel) smoother on the suite's random-walk problem."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from aesmc_amd.testing import particle_gibbs as contract
from tests import particle_gibbs_cases as cases

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 2, 1), (3, 7, 2), (2, 64, 3), (2, 65, 10), (3, 257, 1), (2, 1000, 10), (2, 1024, 16), (2, 300, 17),
          (1, 50, 256), (1, 4097, 10), (1, 8192, 2), (3, 7, 0), (2, 1024, 0), (1, 8192, 0)]


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _launch(device, log_w, u, loc, target, scale):
    """The kernel on NumPy operands -> (idx, flags) as NumPy."""
    provider = _provider()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert provider.read_flags(device) == 0
    idx = provider.conditional_ancestor_index(dev(log_w), dev(u), dev(loc), dev(target), dev(scale))
    flags = provider.read_flags(device)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == log_w.shape
    return idx.cpu().numpy(), flags


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,K,D", SHAPES)
def test_kernel_equals_contract_exactly(hip_device, dtype, B, K, D):
    for number, profile in enumerate(cases.PROFILES):
        if D == 0 and profile in ("tied", "far"):
            continue      # (no transition term: nothing to tie or to move away)
        log_w, u, loc, target, scale = cases.operands(profile, B, K, max(D, 1), dtype, 100 * number + K % 89)
        if D == 0:
            loc = target = scale = None
        elif number % 2:
            scale = scale[:1]      # one value for the whole latent
        want_idx, want_flags = contract.conditional_ancestor_index(log_w, u, loc, target, scale)
        idx, flags = _launch(hip_device, log_w, u, loc, target, scale)
        assert want_flags == 0 and flags == 0, (profile, flags)
        differ = np.argwhere(idx != want_idx)
        assert differ.size == 0, (profile, len(differ), differ[:4], idx[tuple(differ[0])], want_idx[tuple(differ[0])])


@pytest.mark.parametrize("B,K,D", [(2, 300, 5), (1, 4097, 10)])
def test_kernel_equals_backward_sample_on_the_device(hip_device, B, K, D):
    provider = _provider()
    gen = torch.Generator(device=hip_device).manual_seed(K)
    rand = lambda *shape: torch.randn(*shape, device=hip_device, generator=gen)
    log_w, loc, target = rand(B, K), rand(B, K, D), rand(B, D)
    scale = 0.5 + torch.rand(D, device=hip_device, generator=gen)
    u = torch.rand(B, K, device=hip_device, dtype=torch.float64, generator=gen)
    idx = provider.conditional_ancestor_index(log_w, u, loc, target, scale)
    free, _ = provider.backward_sample(log_w, None, None, None, u[:, :K - 1])
    pinned, _ = provider.backward_sample(log_w, loc, target[:, None], scale, u[:, K - 1:])
    assert torch.equal(idx[:, :K - 1], free) and torch.equal(idx[:, K - 1:], pinned)
    plain = provider.conditional_ancestor_index(log_w, u)
    assert torch.equal(plain[:, :K - 1], free) and (plain[:, K - 1] == K - 1).all()
    assert provider.read_flags(hip_device) == 0


def test_views_give_what_dense_copies_give(hip_device):
    provider = _provider()
    B, K, D = 3, 300, 5
    gen = torch.Generator(device=hip_device).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=hip_device, generator=gen)
    log_w = rand(B, K)
    loc_kb = rand(K, B, D)                       # stored [K,B,D]
    target_big = rand(B, 9, D + 4)
    scale = 0.5 + torch.rand(D, device=hip_device, generator=gen)
    u = torch.rand(B, K, device=hip_device, dtype=torch.float64, generator=gen)
    loc, target = loc_kb.transpose(0, 1), target_big[:, 4, 2:2 + D]
    assert not loc.is_contiguous() and not target.is_contiguous()
    for s in (scale, scale[:1], scale[0]):
        dense = provider.conditional_ancestor_index(log_w, u, loc.contiguous(), target.contiguous(), s.clone())
        views = provider.conditional_ancestor_index(log_w, u, loc, target, s)
        assert torch.equal(dense, views)
        want, _ = contract.conditional_ancestor_index(log_w.cpu().numpy(), u.cpu().numpy(), loc.cpu().numpy(),
                                                      target.cpu().numpy(), s.reshape(-1).cpu().numpy())
        assert np.array_equal(views.cpu().numpy(), want)
    # a [B,K] latent is D = 1; a [B,K,2,3] one is D = 6
    flat = provider.conditional_ancestor_index(log_w, u, loc[..., 0], target[..., 0], scale[:1])
    same = provider.conditional_ancestor_index(log_w, u, loc[..., :1], target[..., :1], scale[:1])
    assert torch.equal(flat, same)
    loc6, target6 = rand(B, K, 2, 3), rand(B, 2, 3)
    six = provider.conditional_ancestor_index(log_w, u, loc6, target6, scale[:1])
    same = provider.conditional_ancestor_index(log_w, u, loc6.reshape(B, K, 6), target6.reshape(B, 6), scale[:1])
    assert torch.equal(six, same)
    assert provider.read_flags(hip_device) == 0


def test_bad_rows_flag_and_leave_the_others_alone(hip_device):
    B, K, D = 4, 300, 3
    log_w, u, loc, target, scale = cases.operands("unit", B, K, D, np.float32, 5)
    clean, flags = _launch(hip_device, log_w, u, loc, target, scale)
    assert flags == 0 and (clean < K).all()

    def check(bad_log_w, bad_loc, bad_target, affected, bit):
        want = contract.conditional_ancestor_index(bad_log_w, u, bad_loc, bad_target, scale)
        idx, flags = _launch(hip_device, bad_log_w, u, bad_loc, bad_target, scale)
        assert flags == bit == want[1]
        assert (idx[affected] == K).all() and (idx[~affected] == clean[~affected]).all()
        assert np.array_equal(idx, want[0])
        assert _provider().read_flags(hip_device) == 0                              # the status word is clear afterwards

    row = lambda b: np.ones((B, K), dtype=bool) & (np.arange(B) == b)[:, None]
    slot = lambda b: row(b) & (np.arange(K) == K - 1)[None, :]
    nan_w = log_w.copy()
    nan_w[1, 70] = np.nan
    check(nan_w, loc, target, row(1), contract.FLAG_NAN_LOG_WEIGHT)
    dead = log_w.copy()
    dead[3] = -np.inf
    check(dead, loc, target, row(3), contract.FLAG_DEGENERATE_ROW)
    hot = log_w.copy()
    hot[0, 0] = np.inf
    check(hot, loc, target, row(0), contract.FLAG_DEGENERATE_ROW)
    nan_loc = loc.copy()
    nan_loc[2, 299, 1] = np.nan
    check(log_w, nan_loc, target, slot(2), contract.FLAG_NAN_LOG_WEIGHT)      # only the pinned slot
    nan_target = target.copy()
    nan_target[0, 2] = np.nan
    check(log_w, loc, nan_target, slot(0), contract.FLAG_NAN_LOG_WEIGHT)
    lost = loc.copy()
    lost[1] = np.inf                                                          # every score -inf: no finite maximum
    check(log_w, lost, target, slot(1), contract.FLAG_DEGENERATE_ROW)
    idx, flags = _launch(hip_device, dead, u, None, None, None)
    assert flags == contract.FLAG_DEGENERATE_ROW and (idx[3] == K).all() and (idx[:3, K - 1] == K - 1).all()


def test_index_frequencies_are_the_categorical(hip_device):
    """Independent of the contract: the same two rows of log-weights stacked 4096 times, fresh uniforms in every copy —
    the free slots' counts are (K - 1) * 4096 * softmax(log_w), the pinned slot's 4096 * softmax(s), within 5 sigma + 1."""
    provider = _provider()
    B, K, D, N = 2, 16, 2, 4096
    gen = torch.Generator(device=hip_device).manual_seed(1)
    log_w = torch.randn(B, K, device=hip_device, generator=gen)
    loc = torch.randn(B, K, D, device=hip_device, generator=gen)
    point = torch.randn(B, D, device=hip_device, generator=gen)
    scale = torch.tensor([0.8], device=hip_device)
    u = torch.rand(N * B, K, device=hip_device, dtype=torch.float64, generator=gen)
    idx = provider.conditional_ancestor_index(log_w.repeat(N, 1), u, loc.repeat(N, 1, 1), point.repeat(N, 1), scale)
    assert provider.read_flags(hip_device) == 0
    idx = idx.reshape(N, B, K).cpu().numpy()
    s = log_w.double() - 0.5 * (((point.double()[:, None] - loc.double()) / scale.double()) ** 2).sum(-1)
    p_free = torch.softmax(log_w.double(), dim=1).cpu().numpy()
    p_pinned = torch.softmax(s, dim=1).cpu().numpy()
    for b in range(B):
        for draws, p in ((idx[:, b, :K - 1].reshape(-1), p_free[b]), (idx[:, b, K - 1], p_pinned[b])):
            counts = np.bincount(draws, minlength=K)
            assert counts.sum() == len(draws) and len(counts) == K
            sigma = np.sqrt(len(draws) * p * (1 - p))
            assert (np.abs(counts - len(draws) * p) <= 5 * sigma + 1).all(), (counts, len(draws) * p)


# ---- through the API ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem(hip_device):
    """The contract LGSSM (d = 3, B = 4, T = 6), its observations and a reference path, shared and left unchanged."""
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(3, affine=True).tune_proposal().to(hip_device)
    observations = model.simulate(6, 4, seed=1)
    gen = torch.Generator().manual_seed(5)
    reference = [torch.randn(4, 3, generator=gen).to(hip_device) for _ in range(6)]
    return model, observations, reference


def _callables(model, form, hip_device):
    """(transition, proposal) of the contract model with the transition in one of two forms, the scale per dimension."""
    from aesmc_amd import state
    from aesmc_amd.linear_gaussian import AffineNormal
    full = state.BatchShapeMode.FULLY_EXPANDED
    offset = torch.linspace(-0.2, 0.2, 3, device=hip_device)
    scale = torch.tensor([0.9, 1.0, 1.2], device=hip_device)

    def transition(previous_latents=None, time=None, previous_observations=None):
        if form == "affine_normal":
            return state.set_batch_shape_mode(AffineNormal(previous_latents[-1], model.A, scale, offset=offset), full)
        return state.set_batch_shape_mode(Normal(previous_latents[-1] @ model.A.t() + offset, scale), full)

    return transition, scale


def _uniforms(T, B, K, device, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(B, K if t < T - 1 else 1, dtype=torch.float64, generator=gen).to(device) for t in range(T)]


@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul"])
@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_conditional_smc_equals_the_numpy_pass(hip_device, problem, ancestor_sampling, form):
    from aesmc_amd import particle_gibbs
    model, observations, reference = problem
    transition, scale = _callables(model, form, hip_device)
    T, B, K, d = 6, 4, 33, 3
    uniforms = _uniforms(T, B, K, hip_device)
    path, particles = particle_gibbs.conditional_smc(
        observations, model.initial, transition, model.emission, model.proposal, K, reference,
        ancestor_sampling=ancestor_sampling, uniforms=uniforms, return_particles=True)
    latents, log_weights = particles["latents"], particles["log_weights"]
    # the model's locations as the device forms them (K8's chain for the AffineNormal, the library's product else)
    with torch.no_grad():
        locations = [transition(previous_latents=latents[:t + 1], time=t + 1,
                                previous_observations=observations[:t + 1]).loc.cpu().numpy() for t in range(T - 1)]
    want, stored, ancestral, indices = contract.conditional_pass(
        [x.cpu().numpy() for x in latents], [w.cpu().numpy() for w in log_weights], lambda t: locations[t],
        scale.cpu().numpy(), [x.cpu().numpy() for x in reference], [u.cpu().numpy() for u in uniforms], ancestor_sampling)
    rows = torch.arange(B, device=hip_device)
    for t in range(T):
        assert path[t].shape == (B, d) and not path[t].requires_grad and latents[t].shape == (B, K, d)
        assert torch.equal(latents[t][:, K - 1], reference[t])                       # bitwise
        assert particles["indices"][t].dtype == torch.int64
        assert np.array_equal(particles["indices"][t].cpu().numpy(), indices[t]), (form, t)
        assert torch.equal(path[t], latents[t][rows, particles["indices"][t]])       # the walk back
        assert np.array_equal(path[t].cpu().numpy(), want[t])
        if t < T - 1:
            assert particles["ancestral_indices"][t].dtype == torch.int64
            assert np.array_equal(particles["ancestral_indices"][t].cpu().numpy(), ancestral[t]), (form, t)
            assert torch.equal(particles["indices"][t],
                               particles["ancestral_indices"][t][rows, particles["indices"][t + 1]])
            if not ancestor_sampling:
                assert (particles["ancestral_indices"][t][:, K - 1] == K - 1).all()


@pytest.mark.parametrize("form", ["affine_normal", "normal_of_matmul"])
@pytest.mark.parametrize("ancestor_sampling", [True, False])
def test_conditional_smc_properties(hip_device, problem, ancestor_sampling, form):
    from aesmc_amd import particle_gibbs, state
    model, observations, reference = problem
    transition, scale = _callables(model, form, hip_device)
    run = lambda K, **kw: particle_gibbs.conditional_smc(observations, model.initial, transition, model.emission,
                                                         model.proposal, K, reference,
                                                         ancestor_sampling=ancestor_sampling, **kw)
    path = run(1)                                                              # one particle: the reference exactly
    assert all(torch.equal(a, b) for a, b in zip(path, reference))
    one = particle_gibbs.conditional_smc(observations[:1], model.initial, transition, model.emission, model.proposal, 9,
                                         reference[:1], ancestor_sampling=ancestor_sampling)
    assert len(one) == 1 and one[0].shape == reference[0].shape
    np.random.seed(4)
    before = np.random.get_state()
    torch.manual_seed(6)
    first = run(33)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    torch.manual_seed(6)
    again = run(33)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    other = run(33)
    assert not all(torch.equal(a, b) for a, b in zip(first, other))
    launches = []
    provider = _provider()
    original = provider.conditional_ancestor_index
    provider.conditional_ancestor_index = lambda *a, **kw: launches.append(1) or original(*a, **kw)
    try:
        with pytest.raises(NotImplementedError, match="num_particles = 8193"):
            run(8193)
        assert launches == []

        def particle_scale(previous_latents=None, time=None, previous_observations=None):
            loc = previous_latents[-1] @ model.A.t()
            return state.set_batch_shape_mode(Normal(loc, torch.ones_like(loc)), state.BatchShapeMode.FULLY_EXPANDED)

        sweep = lambda: particle_gibbs.conditional_smc(observations, model.initial, particle_scale, model.emission,
                                                       model.proposal, 9, reference, ancestor_sampling=ancestor_sampling)
        if ancestor_sampling:
            with pytest.raises(NotImplementedError, match="particle-dependent"):
                sweep()
            assert launches == []
        else:
            assert sweep()[0].shape == reference[0].shape
    finally:
        del provider.conditional_ancestor_index
    assert provider.read_flags(hip_device) == 0


def test_posterior_against_the_exact_smoother(hip_device):
    """The scalar random walk of test_gpu_backward_simulation.py::test_smoothed_posterior_against_the_exact_smoother
    (m0 = 0, p0 = 100, q = 25, r = 64, the same y) cut to its first 25 steps, bootstrap proposal, float32: B = 256 chains
    of K = 8 particles, every chain started at y + 60, 40 sweeps of which 10 are discarded; chains and sweeps pooled
    against the Rauch-Tung-Striebel recursion.  With ancestor sampling: RMSE of the means < 0.25, mean relative variance
    error < 0.05, more than half of the kept sweeps replace x_0; plain conditional SMC on the same budget replaces x_0 in
    fewer than 5 % of its sweeps and its RMSE is larger.  The bounds are from the NumPy contract alone on this problem
    (tests/test_particle_gibbs_contract.py::test_numpy_particle_gibbs_against_the_exact_smoother: 0.057 - 0.080, 0.014 -
    0.019, 0.629 - 0.636 with ancestor sampling; replacement 0.0028 - 0.0038, RMSE 1.05 - 1.33 without)."""
    from aesmc_amd import particle_gibbs, state
    Modes = state.BatchShapeMode
    y = cases.data()
    smooth_m, smooth_p = contract.rts_smoother(y, cases.M0, cases.P0, cases.Q, cases.R)
    T, B, K = cases.STEPS, cases.CHAINS, cases.PARTICLES
    dev_t = lambda v: torch.tensor(v, device=hip_device, dtype=torch.float32)
    m0, sd0, sd_q, sd_r = dev_t(cases.M0), dev_t(np.sqrt(cases.P0)), dev_t(np.sqrt(cases.Q)), dev_t(np.sqrt(cases.R))
    full = Modes.FULLY_EXPANDED

    def initial():
        return Normal(m0, sd0)

    def transition(previous_latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(Normal(previous_latents[-1], sd_q), full)

    def emission(latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(Normal(latents[-1], sd_r), full)

    def proposal(previous_latents=None, time=None, observations=None):
        if time == 0:
            return state.set_batch_shape_mode(Normal(m0, sd0), Modes.NOT_EXPANDED)
        return transition(previous_latents=previous_latents)

    observations = torch.from_numpy(y).float().to(hip_device).unsqueeze(-1).expand(T, B).contiguous()
    start = list((observations + cases.AWAY).unbind(0))

    def figures(ancestor_sampling):
        torch.manual_seed(1)
        out = particle_gibbs.particle_gibbs(observations, initial, transition, emission, proposal, K, cases.SWEEPS,
                                            reference=start, ancestor_sampling=ancestor_sampling, burn_in=cases.BURN_IN)
        assert len(out) == T and out[0].shape == (B, cases.SWEEPS - cases.BURN_IN)
        paths = torch.stack(out, dim=2).double().cpu().numpy()              # [B, S, T]
        return contract.posterior_figures(paths, smooth_m, smooth_p)

    rmse, variance, replaced = figures(True)
    plain_rmse, plain_variance, plain_replaced = figures(False)
    print("\n[particle gibbs] pgas: rmse {:.4f} var rel err {:.4f} replaced {:.4f}; plain: rmse {:.4f} var rel err {:.4f} "
          "replaced {:.4f}".format(rmse, variance, replaced, plain_rmse, plain_variance, plain_replaced))
    assert rmse < cases.RMSE_BOUND, rmse
    assert variance < cases.VARIANCE_BOUND, variance
    assert replaced > cases.REPLACED_AT_LEAST, replaced
    assert plain_replaced < cases.PLAIN_REPLACED_AT_MOST, plain_replaced
    assert plain_rmse > rmse, (plain_rmse, rmse)
