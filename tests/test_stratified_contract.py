"""Stratified resampling without a GPU: the NumPy contract (aesmc_amd/testing/resampling.py) against the systematic
oracle and against the properties of the scheme, and the package's HOST logic — the `resampling` setting and argument,
the random streams each scheme consumes, the refusals — on CPU tensors through an oracle provider that knows the
[batch_size, num_particles] uniforms of the stratified scheme."""
import numpy as np
import pytest
import torch

from aesmc_amd import _kernels, distributed, inference, losses, settings
from aesmc_amd.testing import models
from aesmc_amd.testing.resampling import FLAG_DEGENERATE_ROW, FLAG_NAN_LOG_WEIGHT, children_end, stratified_ancestor_index
from oracle import kernel_oracle
from tests.oracle_provider import OracleKernels

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 1024, 4096, 4097]


def weights(rng, B, K, dtype, scale):
    return (scale * rng.randn(B, K)).astype(dtype)


# ---- the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", SIZES)
def test_one_uniform_per_row_is_systematic_resampling(K, dtype):
    """With u[b,:] = u[b] the positions are the systematic ones, (u + k) / K — the clamp never binds there for
    u < 1 - 2**-53 K — so the contract must return the systematic oracle's indices exactly, flags included."""
    rng = np.random.RandomState(K)
    for scale in (0.0, 1.0, 5.0):
        log_w = weights(rng, 3, K, dtype, scale)
        u = rng.uniform(size=3)
        u[0] = 0.0                                                     # positions k / K: CDF steps hit exactly at scale 0
        got, flags = stratified_ancestor_index(log_w, np.repeat(u[:, None], K, axis=1))
        want, want_flags = kernel_oracle.ancestor_index(log_w, u)
        np.testing.assert_array_equal(got, want)
        assert flags == want_flags == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", SIZES)
def test_indices_are_sorted_in_range_and_children_counts_follow_the_weights(K, dtype):
    """Sorted along k, inside [0, K), and |N_j - K w_j| < 2: the children of particle j are the positions inside
    (c[j-1], c[j]], an interval of length w_j, and every stratum of width 1 / K holds exactly one position."""
    rng = np.random.RandomState(1000 + K)
    for scale in (0.0, 1.0, 5.0):
        log_w = weights(rng, 4, K, dtype, scale)
        u = rng.uniform(size=(4, K))
        idx, flags = stratified_ancestor_index(log_w, u)
        assert flags == 0
        assert (np.diff(idx, axis=1) >= 0).all()
        assert idx.min() >= 0 and idx.max() < K
        w = np.exp(log_w.astype(np.float64) - log_w.astype(np.float64).max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        counts = np.stack([np.bincount(row, minlength=K) for row in idx])
        assert np.abs(counts - K * w).max() < 2
        ends = children_end(idx)
        np.testing.assert_array_equal(ends, np.cumsum(counts, axis=1))
        assert (ends[:, -1] == K).all()


@pytest.mark.parametrize("K", [1, 2, 3, 64, 257, 4096])
def test_the_clamp_keeps_planted_edge_uniforms_in_range(K):
    """u = 0 everywhere under uniform weights (every position ON a CDF step), and u[b, K-1] = 1 - 2**-53 — whose sum
    with K - 1 rounds to K, the position 1.0 — on a row whose last third has no weight: in range, on a particle of
    positive weight."""
    uniform = np.zeros((2, K))
    idx, flags = stratified_ancestor_index(uniform, np.zeros((2, K)))
    assert flags == 0 and idx.min() >= 0 and idx.max() < K
    if K & (K - 1) == 0:                                               # k / K and the CDF steps j / K are exact: c[k-1] <= pos[k] < c[k]
        np.testing.assert_array_equal(idx[0], np.arange(K))
    rng = np.random.RandomState(K)
    log_w = rng.randn(2, K)
    dead = max(1, K // 3) if K > 1 else 0
    if dead:
        log_w[:, K - dead:] = -np.inf
        log_w[:, 0] = 0.0
    u = rng.uniform(size=(2, K))
    u[:, K - 1] = 1 - 2.0 ** -53
    if K > 1:
        assert (u[:, K - 1] + (K - 1) == K).all()                      # the sum the clamp exists for
    idx, flags = stratified_ancestor_index(log_w, u)
    assert flags == 0 and idx.min() >= 0 and idx.max() < K
    assert np.isfinite(np.take_along_axis(log_w, idx, axis=1)).all()      # nobody descends from a weightless particle
    assert (np.diff(idx, axis=1) >= 0).all()


def test_special_rows_follow_the_systematic_conventions():
    log_w = np.random.RandomState(0).randn(4, 9).astype(np.float32)
    log_w[1, 3] = np.nan
    log_w[2, :] = -np.inf
    log_w[3, 5] = np.inf
    u = np.random.RandomState(1).uniform(size=(4, 9))
    idx, flags = stratified_ancestor_index(log_w, u)
    assert flags == FLAG_NAN_LOG_WEIGHT | FLAG_DEGENERATE_ROW
    assert (idx[1:] == 9).all() and idx[0].max() < 9
    assert kernel_oracle.ancestor_index(log_w, u[:, 0])[1] == flags
    with pytest.raises(ValueError):
        stratified_ancestor_index(log_w, u[:, 0])


# ---- host logic on the oracle provider ------------------------------------------------------------------------------------
class StratifiedOracleKernels(OracleKernels):
    """The suite's oracle provider with the [B,K] case of the uniforms: the stratified contract."""

    def __init__(self):
        super().__init__()
        self.schemes = []

    def ancestor_index(self, log_w, u):
        if not (u.dim() == 2 and tuple(u.shape) == tuple(log_w.shape)):
            self.schemes.append("systematic")
            return super().ancestor_index(log_w, u)
        self.schemes.append("stratified")
        assert u.dtype == torch.float64
        idx, flags = stratified_ancestor_index(log_w.detach().numpy(), u.numpy())
        self._flags |= flags
        out = torch.from_numpy(idx)
        out._aesmc_sorted = True
        return out

    def resample_step(self, log_w, u, payload=None, want_lse=False, want_child_end=False):
        stratified = u.dim() == 2 and tuple(u.shape) == tuple(log_w.shape)
        idx, lse, moved = super().resample_step(log_w, u, None if stratified else payload, want_lse, want_child_end)
        return idx, lse, moved


@pytest.fixture
def stratified_backend():
    provider = StratifiedOracleKernels()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def run_smc(model, observations, K, **kwargs):
    return inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                           return_log_marginal_likelihood=True, return_ancestral_indices=True, **kwargs)


def numpy_state_fingerprint():
    state = np.random.get_state()
    return state[0], state[1].tobytes(), state[2:]


@pytest.mark.parametrize("how", ["argument", "setting"])
def test_infer_resamples_stratified_from_torchs_generator(stratified_backend, how):
    model = models.LgssmNd(2, seed=0)
    observations = model.simulate(5, 3, seed=0)
    np.random.seed(4)
    torch.manual_seed(4)
    numpy_before, torch_before = numpy_state_fingerprint(), torch.get_rng_state().clone()
    if how == "argument":
        out = run_smc(model, observations, 33, resampling="stratified")
    else:
        with settings.override(resampling="stratified"):
            out = run_smc(model, observations, 33)
    assert stratified_backend.schemes == ["stratified"] * 4
    assert len(out["ancestral_indices"]) == 4
    for index in out["ancestral_indices"]:
        assert index.shape == (3, 33) and index.dtype == torch.int64
        assert bool((index[:, 1:] >= index[:, :-1]).all()) and int(index.min()) >= 0 and int(index.max()) < 33
        assert getattr(index, "_aesmc_sorted", False)
    assert bool(torch.isfinite(out["log_marginal_likelihood"]).all())
    assert numpy_state_fingerprint() == numpy_before                   # numpy's RandomState: not consumed
    assert not torch.equal(torch.get_rng_state(), torch_before)         # torch's CPU generator: advanced
    # the same seed again: the same ancestors (the draws are torch's alone)
    torch.manual_seed(4)
    again = run_smc(model, observations, 33, resampling="stratified")
    for a, b in zip(out["ancestral_indices"], again["ancestral_indices"]):
        assert torch.equal(a, b)
    assert settings.current().resampling == "systematic"


def test_a_uniform_feed_overrides_the_stratified_draws(stratified_backend):
    """`uniform_feed` under stratified: float64 [batch_size, num_particles] per step; every step's indices are the
    contract's for the log-weights it resampled and the uniforms the feed handed out."""
    model = models.LgssmNd(2, seed=0)
    observations = model.simulate(4, 2, seed=1)

    class Feed:
        def __init__(self):
            self.rng, self.handed = np.random.RandomState(8), []

        def next(self):
            self.handed.append(self.rng.uniform(size=(2, 17)))
            return torch.from_numpy(self.handed[-1])

    feed = Feed()
    torch.manual_seed(0)
    with inference.uniform_feed(feed):
        out = run_smc(model, observations, 17, resampling="stratified", return_log_weights=True)
    assert len(feed.handed) == 3
    for step, index in enumerate(out["ancestral_indices"]):
        want, _ = stratified_ancestor_index(out["log_weights"][step].detach().numpy(), feed.handed[step])
        np.testing.assert_array_equal(index.numpy(), want)

    class RowFeed:
        def next(self):
            return torch.rand(2, dtype=torch.float64)

    with inference.uniform_feed(RowFeed()), pytest.raises(ValueError, match="stratified"):
        run_smc(model, observations, 17, resampling="stratified")
    with inference.uniform_feed(Feed()), pytest.raises(ValueError, match="systematic"):
        run_smc(model, observations, 17)


def test_sample_ancestral_index_takes_the_scheme(stratified_backend):
    log_weight = torch.randn(5, 40, generator=torch.Generator().manual_seed(0))
    np.random.seed(2)
    torch.manual_seed(2)
    numpy_before = numpy_state_fingerprint()
    index = inference.sample_ancestral_index(log_weight, resampling="stratified")
    assert numpy_state_fingerprint() == numpy_before
    torch.manual_seed(2)
    want, _ = stratified_ancestor_index(log_weight.numpy(), torch.rand((5, 40), dtype=torch.float64).numpy())
    np.testing.assert_array_equal(index.numpy(), want)
    with settings.override(resampling="stratified"):
        torch.manual_seed(2)
        assert torch.equal(inference.sample_ancestral_index(log_weight), index)
    # the default: numpy's block, as before
    np.random.seed(2)
    index = inference.sample_ancestral_index(log_weight)
    np.random.seed(2)
    want, _ = kernel_oracle.ancestor_index(log_weight.numpy(), inference.draw_uniform_block(5))
    np.testing.assert_array_equal(index.numpy(), want)
    assert stratified_backend.schemes == ["stratified", "stratified", "systematic"]


def test_an_unknown_scheme_is_a_value_error(stratified_backend):
    model = models.LgssmNd(2, seed=0)
    observations = model.simulate(3, 2, seed=0)
    with pytest.raises(ValueError, match="resampling"):
        run_smc(model, observations, 8, resampling="multinomial")
    with pytest.raises(ValueError, match="resampling"):
        inference.sample_ancestral_index(torch.zeros(2, 8), resampling="residual")
    with pytest.raises(ValueError, match="resampling"):
        settings.set_default(resampling="multinomial")
    with pytest.raises(ValueError, match="resampling"):
        with settings.override(resampling=""):
            pass
    assert settings.current().resampling == "systematic"
    assert settings.Settings().resampling == "systematic"


def test_stratified_inside_a_shard_is_refused(stratified_backend):
    model = models.LgssmNd(2, seed=0)
    observations = model.simulate(3, 2, seed=0)
    with distributed.shard_scope(4, 0, 2):
        with pytest.raises(NotImplementedError, match="shard"):
            run_smc(model, observations, 8, resampling="stratified")
        with settings.override(resampling="stratified"), pytest.raises(NotImplementedError, match="shard"):
            inference.sample_ancestral_index(torch.zeros(2, 8))
        run_smc(model, observations, 8)                                  # systematic: as before


def test_the_default_run_consumes_numpys_uniforms_exactly_as_before(stratified_backend):
    """Nothing named: systematic, one `draw_uniform_block(batch_size)` per resampling step from numpy's RandomState —
    the run ends with the RandomState where T - 1 such draws (and the model's own, none here) leave it, and every
    step's indices are the systematic oracle's for those blocks."""
    model = models.LgssmNd(2, seed=0)
    observations = model.simulate(5, 3, seed=0)
    np.random.seed(9)
    torch.manual_seed(9)
    out = run_smc(model, observations, 21, return_log_weights=True)
    after = numpy_state_fingerprint()
    np.random.seed(9)
    blocks = [inference.draw_uniform_block(3) for _ in range(4)]
    assert numpy_state_fingerprint() == after
    assert stratified_backend.schemes == ["systematic"] * 4
    for step, index in enumerate(out["ancestral_indices"]):
        want, _ = kernel_oracle.ancestor_index(out["log_weights"][step].detach().numpy(), blocks[step])
        np.testing.assert_array_equal(index.numpy(), want)


def test_get_loss_picks_the_setting_up(stratified_backend):
    model = models.LgssmNd(2, seed=0)
    observations = model.simulate(4, 2, seed=0)
    np.random.seed(1)
    numpy_before = numpy_state_fingerprint()
    with settings.override(resampling="stratified"):
        torch.manual_seed(1)
        loss = losses.get_loss(observations, 16, "aesmc", model.initial, model.transition, model.emission, model.proposal)
    assert bool(torch.isfinite(loss)) and stratified_backend.schemes == ["stratified"] * 3
    assert numpy_state_fingerprint() == numpy_before
