"""GPU tests of stratified resampling: the HIP kernel (aesmc_resample_step_stratified, through the provider) against
the NumPy contract of aesmc_amd/testing/resampling.py — exactly — and the scheme through every layer above it: the
provider's by-products and refusals, `infer` on the fused forward / backward routes, the hipGraph capture, and the
statistics a resampler must reproduce."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd import _lib, graphs, inference, losses, settings, state, statistics
from aesmc_amd.state import BatchShapeMode as Modes
from aesmc_amd.testing import models
from aesmc_amd.testing.resampling import children_end, stratified_ancestor_index

pytestmark = pytest.mark.gpu

F32_TOL, F64_TOL = (2e-6, 2e-6), (1e-13, 1e-13)      # tests/test_gpu_kernels.py's bars for the row log-sum-exp
LIMIT = 32768                                         # aesmc_ancestor_index_lds_max_particles(); asserted below
SHAPES = [(1, 1), (2, 2), (3, 7), (5, 64), (4, 65), (4, 129), (3, 1000), (3, 1024), (2, 4096), (2, 4097), (2, 8191),
          (2, 16384), (2, LIMIT), (3, LIMIT + 1500), (300, 50)]
BELOW_ONE = 1 - 2.0 ** -53


@pytest.fixture(scope="module")
def kernels(hip_device):
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip" and provider.lds_max_particles == LIMIT
    provider.read_flags(hip_device)
    return provider


def dev(array, device):
    return torch.from_numpy(np.ascontiguousarray(array)).to(device)


def weight_profiles(rng, B, K):
    """The profiles of test_ancestor_index_randomised_stress, each once: (name, float64 log-weights [B,K])."""
    out = [("scale %g" % scale, rng.randn(B, K) * scale) for scale in (0.0, 0.1, 1.0, 10.0, 100.0)]
    out.append(("ties", np.round(rng.randn(B, K) * 2) / 2))
    hole = rng.randn(B, K)
    if K > 4:
        lo = rng.randint(0, K - 2)
        hole[:, lo:lo + max(1, K // 3)] = -np.inf            # a stretch without weight
        hole[:, (lo + K // 2) % K] = 0.0                        # ... but never a dead row
    out.append(("-inf stretch", hole))
    dominant = rng.randn(B, K)
    dominant[:, rng.randint(0, K)] += 50.0
    out.append(("dominant", dominant))
    for name, at in (("first", 0), ("middle", K // 2), ("last", K - 1)):
        hot = np.full((B, K), -np.inf)
        hot[:, at] = 0.0
        out.append(("one-hot " + name, hot))
    return out


def planted_uniforms(rng, B, K):
    """Uniforms in [0, 1) with exact 0.0 and 1 - 2**-53 planted, also in the last stratum (whose sum with K - 1 then
    rounds to K: the clamp's case)."""
    u = rng.uniform(size=(B, K))
    for b in range(B):
        where = rng.randint(0, K, size=max(1, K // 16))
        u[b, where[::2]] = 0.0
        u[b, where[1::2]] = BELOW_ONE
        u[b, K - 1] = BELOW_ONE if b % 2 == 0 else 0.0
    u[0, 0] = 0.0
    return u


# ---- the kernel against the contract ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_contract(kernels, hip_device, shape, dtype):
    """Indices and flags exactly; where one workgroup resolves the row, the by-products of the same launch too: the
    children ranges are the counts the indices imply, the row log-sum-exp is K1's to its tolerance."""
    from oracle import c_oracle
    B, K = shape
    rng = np.random.RandomState(K + 7 * B)
    rtol, atol = F32_TOL if dtype == np.float32 else F64_TOL
    for name, log_w in weight_profiles(rng, B, K):
        log_w = log_w.astype(dtype)
        u = planted_uniforms(rng, B, K)
        want, want_flags = stratified_ancestor_index(log_w, u)
        assert want_flags == 0 and want.max() < K
        kernels.read_flags(hip_device)
        got = kernels.ancestor_index(dev(log_w, hip_device), dev(u, hip_device))
        assert getattr(got, "_aesmc_sorted", False)
        got = got.cpu().numpy()
        assert kernels.read_flags(hip_device) == 0, name
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, shape, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        step = kernels.resample_step(dev(log_w, hip_device), dev(u, hip_device), None, want_lse=True, want_child_end=True)
        if K > LIMIT:
            assert step is None
            continue
        idx, lse, moved = step
        assert moved is None
        np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=name)
        np.testing.assert_array_equal(idx._aesmc_child_end.cpu().numpy(), children_end(want), err_msg=name)
        _, want_lse = c_oracle.logweight_lse(log_w)
        np.testing.assert_allclose(lse.cpu().numpy().astype(np.float64), want_lse, rtol=rtol, atol=atol, err_msg=name)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(3, 7), (4, 129), (3, 1000), (3, 1024), (2, 4096), (2, 8191), (2, 16384),
                                   (2, LIMIT + 1500)])
def test_one_uniform_per_row_is_the_systematic_kernel(kernels, hip_device, shape, dtype):
    """u[b] broadcast over the particles through the new entry: the existing kernel's indices bit for bit (rows where the
    systematic kernel itself answers K — none here — would be excluded: the stratified clamp never does)."""
    B, K = shape
    rng = np.random.RandomState(K)
    for scale in (0.0, 1.0, 5.0):
        log_w = (scale * rng.randn(B, K)).astype(dtype)
        u = rng.uniform(size=B)
        u[0] = 0.0
        systematic = kernels.ancestor_index(dev(log_w, hip_device), dev(u, hip_device)).cpu().numpy()
        stratified = kernels.ancestor_index(dev(log_w, hip_device),
                                            dev(np.repeat(u[:, None], K, axis=1), hip_device)).cpu().numpy()
        rows = (systematic < K).all(axis=1)
        assert rows.all()
        np.testing.assert_array_equal(stratified[rows], systematic[rows])


@pytest.mark.parametrize("K", [50, 4096, LIMIT + 1500])
def test_special_rows_flag_and_answer_like_the_contract(kernels, hip_device, K):
    rng = np.random.RandomState(2)
    log_w = rng.randn(4, K).astype(np.float32)
    u = rng.uniform(size=(4, K))
    for plant in ("nan", "dead", "inf", "both"):
        bad = log_w.copy()
        if plant in ("nan", "both"):
            bad[1, K // 3] = np.nan
        if plant in ("dead", "both"):
            bad[2, :] = -np.inf
        if plant == "inf":
            bad[3, K - 1] = np.inf
        want, want_flags = stratified_ancestor_index(bad, u)
        kernels.read_flags(hip_device)
        got = kernels.ancestor_index(dev(bad, hip_device), dev(u, hip_device)).cpu().numpy()
        assert kernels.read_flags(hip_device) == want_flags != 0
        np.testing.assert_array_equal(got, want)
        if K <= LIMIT:
            idx, lse, _ = kernels.resample_step(dev(bad, hip_device), dev(u, hip_device), None, want_lse=True,
                                                want_child_end=True)
            assert kernels.read_flags(hip_device) == want_flags
            np.testing.assert_array_equal(idx.cpu().numpy(), want)
            dead_rows = (want == K).all(axis=1)
            assert (idx._aesmc_child_end.cpu().numpy()[dead_rows] == 0).all()
            np.testing.assert_array_equal(idx._aesmc_child_end.cpu().numpy()[~dead_rows], children_end(want[~dead_rows]))
            want_lse = torch.logsumexp(torch.from_numpy(bad), dim=1).numpy()
            np.testing.assert_allclose(lse.cpu().numpy(), want_lse, rtol=2e-6, atol=2e-6, equal_nan=True)


def test_the_entry_rejects_bad_arguments_before_any_launch(kernels, hip_device):
    lib = kernels._lib
    entry = lib.aesmc_resample_step_stratified
    B, K = 2, 16
    log_w = torch.zeros(B, K, device=hip_device)
    u = torch.rand(B, K, dtype=torch.float64, device=hip_device)
    idx = torch.full((B, K), -7, dtype=torch.int64, device=hip_device)
    stream = kernels._stream(log_w)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    invalid, unsupported, workspace = 1, _lib.ERR_UNSUPPORTED, 4
    assert entry(_lib.F32, None, p(u), p(idx), None, None, None, B, K, None, 0, stream) == invalid
    assert entry(_lib.F32, p(log_w), None, p(idx), None, None, None, B, K, None, 0, stream) == invalid
    assert entry(_lib.F32, p(log_w), p(u), None, None, None, None, B, K, None, 0, stream) == invalid
    assert entry(_lib.F32, p(log_w), p(u), p(idx), None, None, None, -1, K, None, 0, stream) == invalid
    assert entry(_lib.F32, p(log_w), p(u), p(idx), None, None, None, B, -1, None, 0, stream) == invalid
    assert entry(7, p(log_w), p(u), p(idx), None, None, None, B, K, None, 0, stream) == invalid
    big = LIMIT + 1
    lse = torch.zeros(B, device=hip_device)
    # beyond the in-workgroup limit: no by-products, and the indices only through a workspace — nothing is launched for
    # these calls, so the (too small) buffers are never touched
    assert entry(_lib.F32, p(log_w), p(u), p(idx), p(lse), None, None, B, big, None, 0, stream) == unsupported
    assert entry(_lib.F32, p(log_w), p(u), p(idx), None, None, None, B, big, None, 0, stream) == workspace
    assert entry(_lib.F32, p(log_w), p(u), p(idx), None, None, None, 0, K, None, 0, stream) == _lib.OK
    torch.cuda.synchronize()
    assert bool((idx == -7).all())
    with pytest.raises(ValueError):
        kernels.ancestor_index(log_w, torch.rand(B, K + 1, dtype=torch.float64, device=hip_device))
    with pytest.raises(ValueError):
        kernels.ancestor_index(log_w, torch.rand(B, K, dtype=torch.float32, device=hip_device))


# ---- through the provider and `infer` -------------------------------------------------------------------------------------------
class RecordingFeed:
    """A `uniform_feed` that draws [B,K] float64 uniforms on the device from a generator of its own and keeps them."""

    def __init__(self, shape, device, seed):
        self.shape, self.device = shape, device
        self.generator = torch.Generator(device=device).manual_seed(seed)
        self.handed = []

    def next(self):
        self.handed.append(torch.rand(self.shape, dtype=torch.float64, device=self.device, generator=self.generator))
        return self.handed[-1]


def test_a_payload_is_offered_and_gathered_by_the_caller(kernels, hip_device):
    """`resample_step` under stratified has no payload tail: `step_covers` accepts the payload, the launch returns
    `moved is None`, and `infer` still hands out correctly gathered values (torch.gather through the returned indices)."""
    rng = np.random.RandomState(3)
    log_w = dev(rng.randn(3, 200).astype(np.float32), hip_device)
    payload = dev(rng.randn(3, 200, 4).astype(np.float32), hip_device)
    u = torch.rand(3, 200, dtype=torch.float64, device=hip_device)
    assert kernels.step_covers(log_w, payload)
    idx, lse, moved = kernels.resample_step(log_w, u, payload, want_lse=True)
    assert moved is None and lse.shape == (3,)
    want, _ = stratified_ancestor_index(log_w.cpu().numpy(), u.cpu().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), want)

    model = models.LgssmNd(4, dtype=torch.float32).to(hip_device)      # Normal(matmul) callables: they read the values
    observations = model.simulate(3, 2, seed=3)
    offered = []
    real = kernels.resample_step

    def spy(*args, **kwargs):
        out = real(*args, **kwargs)
        payload = args[2] if len(args) > 2 else kwargs.get("payload")
        offered.append((payload is not None, out[2]))
        return out

    kernels.resample_step = spy
    try:
        torch.manual_seed(5)
        with inference.lazy_gather(False):
            out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal,
                                  300, return_original_latents=True, return_ancestral_indices=True,
                                  resampling="stratified")
    finally:
        kernels.resample_step = real
    assert offered == [(True, None), (True, None)]
    originals, (first, second) = out["original_latents"], out["ancestral_indices"]
    gather = lambda x, index: torch.gather(x, 1, index.unsqueeze(-1).expand(-1, -1, x.size(2)))
    assert torch.equal(out["latents"][2], originals[2])
    assert torch.equal(out["latents"][1], gather(originals[1], second))
    assert torch.equal(out["latents"][0], gather(originals[0], torch.gather(first, 1, second)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_every_step_of_infer_is_the_contract(hip_device, dtype):
    """B=3, K=512, T=4 on the linear-Gaussian model with a recording feed: each step's ancestors are the contract's for
    the log-weights of the step before and the uniforms that step was handed."""
    B, K, T = 3, 512, 4
    model = models.LgssmNd(10, dtype=dtype, affine=True).tune_proposal().to(hip_device)
    observations = model.simulate(T, B, seed=3)
    feed = RecordingFeed((B, K), hip_device, seed=4)
    torch.manual_seed(1)
    with inference.uniform_feed(feed), torch.no_grad():
        out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                              return_ancestral_indices=True, return_log_weights=True, resampling="stratified")
    assert len(feed.handed) == T - 1 == len(out["ancestral_indices"])
    for step, index in enumerate(out["ancestral_indices"]):
        want, flags = stratified_ancestor_index(out["log_weights"][step].cpu().numpy(), feed.handed[step].cpu().numpy())
        assert flags == 0
        np.testing.assert_array_equal(index.cpu().numpy(), want)
        assert getattr(index, "_aesmc_sorted", False)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_lazily_resampled_stratified_run_is_the_eagerly_gathered_run(hip_device, grad, dtype):
    """tests/test_gpu_noise_and_lazy_latents.py's comparison under stratified resampling with a fixed feed: the
    propagation launch that fetches its rows through STRATIFIED ancestors against the run that gathers them first —
    latents, ancestors, evidence and gradients identical."""
    from aesmc_amd import _kernels
    provider = _kernels.get()
    runs = {}
    for lazy in (False, True):
        calls = {"propagate_ancestors": 0}
        real_propagate = provider.affine_propagate

        def propagate_spy(*args, **kwargs):
            calls["propagate_ancestors"] += kwargs.get("ancestors") is not None
            return real_propagate(*args, **kwargs)

        state.set_kernel_noise(False)       # this test is about the gather alone: torch draws the noise
        provider.affine_propagate = propagate_spy
        try:
            model = models.LgssmNd(10, dtype=dtype, affine=True).tune_proposal().to(hip_device)
            observations = model.simulate(6, 4, seed=3)
            torch.manual_seed(11)
            feed = RecordingFeed((4, 1300), hip_device, seed=12)
            with torch.set_grad_enabled(grad), inference.lazy_gather(lazy), inference.uniform_feed(feed), \
                    settings.override(resampling="stratified"):
                out = inference.infer("smc", observations, model.initial, model.transition, model.emission,
                                      model.proposal, 1300, return_log_marginal_likelihood=True, return_latents=False,
                                      return_log_weight=not grad, return_ancestral_indices=True,
                                      return_original_latents=True)
            if grad:
                (-out["log_marginal_likelihood"].mean()).backward()
        finally:
            provider.affine_propagate = real_propagate
            state.set_kernel_noise(True)
        runs[lazy] = (out, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, calls)
    (a, grads_a, calls_a), (b, grads_b, calls_b) = runs[False], runs[True]
    assert calls_a["propagate_ancestors"] == 0 and calls_b["propagate_ancestors"] == 5
    assert torch.equal(a["log_marginal_likelihood"], b["log_marginal_likelihood"])
    for x, y in zip(a["original_latents"] + a["ancestral_indices"], b["original_latents"] + b["ancestral_indices"]):
        assert torch.equal(x, y)
    assert torch.equal(a["last_latent"], b["last_latent"])
    assert sorted(grads_a) == sorted(grads_b) and (not grad or grads_a)
    for name in grads_a:
        assert torch.equal(grads_a[name], grads_b[name]), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_folded_gather_backward_takes_stratified_children_ranges(hip_device, dtype):
    """`fold_gather_backward(True)` — K14 summing each particle's children through the ranges the STRATIFIED launch
    wrote — against the run where every step's gather has a backward launch of its own: same loss, gradients to the
    bars of the systematic comparison (2e-4 / 1e-10 of the largest entry)."""
    from aesmc_amd import _kernels
    provider = _kernels.get()
    T, B, K = 5, 3, 1500
    runs = {}
    for fold in (False, True):
        calls = {"with_children": 0}
        real_sb = provider.affine_step_backward

        def sb_spy(*args, **kwargs):
            calls["with_children"] += kwargs.get("child_grad") is not None
            return real_sb(*args, **kwargs)

        provider.affine_step_backward = sb_spy
        try:
            model = models.LgssmNd(10, dtype=dtype, affine=True).tune_proposal().to(hip_device)
            observations = model.simulate(T, B, seed=3)
            torch.manual_seed(11)
            feed = RecordingFeed((B, K), hip_device, seed=12)
            with inference.fold_gather_backward(fold), inference.uniform_feed(feed), \
                    settings.override(resampling="stratified"):
                loss = losses.get_loss(observations, K, "aesmc", model.initial, model.transition, model.emission,
                                       model.proposal)
                loss.backward()
        finally:
            provider.affine_step_backward = real_sb
        runs[fold] = (loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, calls)
    (loss_a, grads_a, calls_a), (loss_b, grads_b, calls_b) = runs[False], runs[True]
    assert torch.equal(loss_a, loss_b)
    assert calls_a["with_children"] == 0 and calls_b["with_children"] == T - 2
    assert sorted(grads_a) == sorted(grads_b) and grads_a
    tolerance = 2e-4 if dtype == torch.float32 else 1e-10
    for name in grads_a:
        scale = max(1.0, float(grads_a[name].abs().max()))
        assert float((grads_a[name] - grads_b[name]).abs().max()) <= tolerance * scale, name


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def test_stratified_infer_against_a_kalman_filter(hip_device):
    """test_infer_against_a_kalman_filter's model, data and bounds under stratified resampling: the filtering mean and
    variance at the last step and log Z agree with the closed-form scalar Kalman filter."""
    T, K = 100, 1000
    rng = np.random.RandomState(0)
    grid = np.linspace(0, 3 * np.pi, T)
    y = 40 * (np.sin(grid) + 0.2 * rng.randn(T))
    m0, p0, q, r = 0.0, 100.0, 25.0, 64.0          # x_0 ~ N(m0, p0), x_t = x_{t-1} + N(0, q), y_t = x_t + N(0, r)
    mean, var, loglik = m0, p0, 0.0
    for t in range(T):                               # scalar Kalman filter
        if t > 0:
            var = var + q
        s = var + r
        loglik += -0.5 * (np.log(2 * np.pi * s) + (y[t] - mean) ** 2 / s)
        gain = var / s
        mean, var = mean + gain * (y[t] - mean), (1 - gain) * var
    dev_t = lambda v: torch.tensor(v, device=hip_device, dtype=torch.float32)
    full = Modes.FULLY_EXPANDED

    def initial():
        return torch.distributions.Normal(dev_t(m0), dev_t(np.sqrt(p0)))

    def transition(previous_latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(torch.distributions.Normal(previous_latents[-1], dev_t(np.sqrt(q))), full)

    def emission(latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(torch.distributions.Normal(latents[-1], dev_t(np.sqrt(r))), full)

    def proposal(previous_latents=None, time=None, observations=None):
        if time == 0:
            return state.set_batch_shape_mode(torch.distributions.Normal(dev_t(m0), dev_t(np.sqrt(p0))), Modes.NOT_EXPANDED)
        return transition(previous_latents=previous_latents)

    observations = torch.from_numpy(y).unsqueeze(-1).float().to(hip_device)      # [T, 1]: time first, batch of one
    torch.manual_seed(1)
    numpy_before = np.random.get_state()[1].tobytes()
    smc = inference.infer("smc", observations, initial, transition, emission, proposal, K,
                          return_log_marginal_likelihood=True, resampling="stratified")
    assert np.random.get_state()[1].tobytes() == numpy_before
    got_mean = statistics.empirical_mean(smc["latents"][-1], smc["log_weight"])[0].item()
    got_var = statistics.empirical_variance(smc["latents"][-1], smc["log_weight"])[0].item()
    ess = statistics.ess(smc["log_weight"])[0].item()
    assert abs(got_mean - mean) < 5 * np.sqrt(var / ess) + 0.5, (got_mean, mean, ess)
    assert 0.5 * var < got_var < 1.6 * var, (got_var, var)
    assert abs(smc["log_marginal_likelihood"][0].item() - loglik) < 3.0, (smc["log_marginal_likelihood"], loglik)


def test_stratified_sampler_frequencies(hip_device):
    """The reference's TestSampleAncestralIndex :: test_sampler under the stratified scheme."""
    for shape in [(2, 3), (1, 2), (2, 1)]:
        index = inference.sample_ancestral_index(torch.rand(*shape, device=hip_device), resampling="stratified")
        assert index.size() == torch.Size(shape) and index.dtype == torch.int64 and index.device == hip_device
    weight, trials = [0.2, 0.3, 0.5], 10000
    torch.manual_seed(0)
    index = inference.sample_ancestral_index(
        torch.log(torch.Tensor(weight)).unsqueeze(0).expand(trials, len(weight)).to(hip_device), resampling="stratified")
    frequencies = [(index == i).float().sum().item() / (trials * len(weight)) for i in range(len(weight))]
    np.testing.assert_allclose(frequencies, weight, atol=1e-2)


# ---- hipGraph ---------------------------------------------------------------------------------------------------------------------
def test_graphed_loss_under_stratified_resampling(hip_device):
    """Capture at B=4, K=256, T=3 with backward: no static uniform feed (the draws are captured torch.rand calls),
    the built-in replay-against-eager verification passes, and two replays draw different uniforms."""
    model = models.LgssmNd(3, seed=0, dtype=torch.float64, validate_args=False, affine=True).to(hip_device)
    observations = model.simulate(3, 4, seed=1)
    parts = (model.initial, model.transition, model.emission, model.proposal)
    torch.manual_seed(3)
    numpy_before = np.random.get_state()[1].tobytes()
    with settings.override(resampling="stratified"):
        graphed = graphs.GraphedLoss(observations, 256, "aesmc", *parts, backward=True, verify_replays=2)
    assert graphed.feed is None and graphed.resampling == "stratified"
    first = graphed().clone()                      # outside the block: the captured scheme stays
    first_grads = [p.grad.clone() for p in model.parameters()]
    second = graphed().clone()
    assert bool(torch.isfinite(first)) and bool(torch.isfinite(second))
    assert float((first - second).abs()) > 0
    assert any(not torch.equal(p.grad, g) for p, g in zip(model.parameters(), first_grads))
    problems, _ = graphed.reverify(observations)
    assert problems == []
    graphed.check()
    assert np.random.get_state()[1].tobytes() == numpy_before
