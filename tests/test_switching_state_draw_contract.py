"""CPU checks of the simulation smoother of switching linear-Gaussian models (kernel K47, aesmc_switching_state_draw): its NumPy
contract (aesmc_amd/testing/switching_state_draw.py) against dense np.linalg and the dense state smoother — exactly, through
the affine structure of the pass, every noise value counting —, the degenerate models the dropping rule exists for, the index
and time conventions, the C entry's status codes and the host logic of `aesmc_amd.rao_blackwell.switching_sample_states` on a
provider double.

Pivots near a threshold: every case asserts, from the contract alone, that each pivot of both factorisations lies further
from its threshold than 4 times its running bound (`clearance` > 1), so a device keeps and drops the same columns."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_missing as missing
from aesmc_amd.testing import switching_state_draw as draw
from tests.oracle_provider import OracleKernels

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
SHAPES = [(1, 1, 1), (3, 2, 1), (2, 4, 3), (16, 8, 8)]
# The largest deviation of the float64 contract from the dense smoother over SHAPES in `exactness_case`, plain and masked,
# measured on the CPU: means 1.5e-15, covariances 7.0e-16, lag-one cross-covariances 1.5e-15 (all at (16, 8, 8)).  Times 8:
# the margin for a device's fused multiply-adds and reassociation.
MEASURED = {"means": 1.5e-15, "covariances": 7.0e-16, "cross_covariances": 1.5e-15}
EXACTNESS_TOLERANCE = {key: 8 * value for key, value in MEASURED.items()}


def _shared_path(rng, T, B, N, M):
    """One regime path per batch row, shared by its N trajectories."""
    return [np.ascontiguousarray(np.broadcast_to(rng.integers(0, M, (B, 1)), (B, N))).astype(np.int32) for _ in range(T)]


def exactness_case(M, D, Dy, masked, T=3):
    """(model, regimes, observations, observed, noise) of the exactness test: one path, N = T D + 1 trajectories that share
    it; trajectory 0 has zero noise, trajectory 1 + k the k-th unit vector of the stacked noise."""
    rng = np.random.default_rng([M, D, Dy, T, 47])
    model = contract.example_model(M, D, Dy, seed=1)
    N = T * D + 1
    regimes = _shared_path(rng, T, 1, N, M)
    observations = [rng.standard_normal((1, Dy)) for _ in range(T)]
    observed = None
    if masked:
        observed = missing.example_masks(T, 1, Dy, seed=3)
        observations = [np.where(mask, y, np.nan) for y, mask in zip(observations, observed)]
    noise = np.zeros((T, 1, N, D))
    for k in range(T * D):
        noise[k // D, 0, 1 + k, k % D] = 1.0
    return model, regimes, observations, observed, list(noise)


def affine_moments(states, D):
    """(mu [T,D], diagonal blocks [T,D,D], lag-one blocks [T-1,D,D], rows at t+1) of the affine map the draws of
    `exactness_case` span: mu = z(0), the columns of W are z(1+k) - z(0), the blocks those of W W^T."""
    z = np.stack(states)[:, 0]                                         # [T,N,D]
    T = z.shape[0]
    W = (z[:, 1:] - z[:, :1]).transpose(0, 2, 1).reshape(T * D, T * D)
    full = W @ W.T
    at = lambda t: slice(t * D, (t + 1) * D)
    return z[:, 0], np.stack([full[at(t), at(t)] for t in range(T)]), \
        np.stack([full[at(t + 1), at(t)] for t in range(T - 1)]) if T > 1 else np.zeros((0, D, D))


def dense_moments(model, regimes, observations, observed):
    """The same three from the dense side: `exact_state_smoother`, under a mask `switching_missing.switching_state_pass`."""
    D = model["A"].shape[-1]
    if observed is None:
        return contract.exact_state_smoother(model, [int(r[0, 0]) for r in regimes], [y[0] for y in observations])
    out = missing.switching_state_pass(model, [r[:, :1] for r in regimes], [np.nan_to_num(y) for y in observations], observed)
    return (np.stack([m[0, 0] for m in out["means"]]), np.stack([contract.unpack(c[0, 0], D) for c in out["covariances"]]),
            np.stack([x[0, 0] for x in out["cross_covariances"]]))


# ---- 1. the step against dense np.linalg ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(1, 1), (3, 2), (2, 4), (16, 8)])
def test_the_step_is_the_dense_conditioning(M, D):
    """G = P A^T S^-1 and chol(P - G A P) read off the step: with m = 0 and b = 0 the draw from z_next = e_k, eps = 0 is
    column k of G, and the draw from z_next = 0, eps = e_k column k of the factor.  Within 2 x `state_draw_step_bound`."""
    rng = np.random.default_rng([M, D, 1])
    model = contract.example_model(M, D, 1, seed=4)
    model = dict(model, b=np.zeros_like(model["b"]))
    B, N = 2, 2 * D
    root = rng.standard_normal((B, 1, D, D))
    full = root @ np.swapaxes(root, -1, -2) / D + 0.1 * np.eye(D)
    cov = np.ascontiguousarray(np.broadcast_to(contract.pack(full), (B, N, D * (D + 1) // 2)))
    regime = np.ascontiguousarray(np.broadcast_to(rng.integers(0, M, (B, 1)), (B, N))).astype(np.int32)
    z_next, eps = np.zeros((B, N, D)), np.zeros((B, N, D))
    for k in range(D):
        z_next[:, k, k] = 1.0
        eps[:, D + k, k] = 1.0
    args = (model, regime, np.zeros((B, N, D)), cov, z_next, eps)
    z, flags, margin = draw.state_draw_step(*args)
    bound, clearance = draw.state_draw_step_bound(*args)
    assert flags == 0 and clearance > 1 and margin > 0.01
    worst = 0.0
    for b in range(B):
        A, P = model["A"][regime[b, 0]], full[b, 0]
        S = A @ P @ A.T + np.diag(model["q"][regime[b, 0]] ** 2)
        G = P @ A.T @ np.linalg.inv(S)
        factor = np.linalg.cholesky(P - G @ A @ P)
        for got, want, allowed in ((z[b, :D].T, G, bound[b, :D].T), (z[b, D:].T, factor, bound[b, D:].T)):
            worst = max(worst, float((np.abs(got - want) / (2 * allowed + 1e-300)).max()))
            assert (np.abs(got - want) <= 2 * allowed).all()
    print("largest error over 2 x bound", worst)


@pytest.mark.parametrize("following", [True, False])
@pytest.mark.parametrize("M,D", [(1, 1), (3, 2), (2, 4), (16, 8)])
def test_the_bound_holds_against_extended_precision(M, D, following):
    rng = np.random.default_rng([M, D, 2])
    B, N = 2, 5
    model, state, _, _, _ = contract.example_step(B, N, M, D, 1, seed=2)
    _, mean, cov = state
    regime = rng.integers(0, M, (B, N)).astype(np.int32) if following else None
    z_next = rng.standard_normal((B, N, D)) if following else None
    args = (model, regime, mean, cov, z_next, rng.standard_normal((B, N, D)))
    z, flags, _ = draw.state_draw_step(*args)
    wide, _, _ = draw.state_draw_step(*args, dtype=np.longdouble)
    bound, clearance = draw.state_draw_step_bound(*args)
    assert flags == 0 and clearance > 1
    error = np.abs(z.astype(np.longdouble) - wide).astype(np.float64)
    print("largest error", error.max(), "largest bound", bound.max())
    assert (error <= bound / 2).all() and bound.max() < 1e-11


# ---- 2. exactness, every noise value counting -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,D,Dy", SHAPES)
def test_the_pass_spans_the_exact_smoother(M, D, Dy, masked):
    """The pass is affine in the noise: z = mu + W eps.  mu must be the smoothed means, the diagonal blocks of W W^T the smoothed
    covariances and its lag-one blocks the cross-covariances (rows at t+1) — a wrong gain, factor, sign or time index shows
    in one of them."""
    model, regimes, observations, observed, noise = exactness_case(M, D, Dy, masked)
    out = draw.state_draw_pass(model, regimes, observations, noise, observed)
    assert out["flags"] == 0 and out["clearance"] > 1
    got = dict(zip(("means", "covariances", "cross_covariances"), affine_moments(out["states"], D)))
    want = dict(zip(("means", "covariances", "cross_covariances"), dense_moments(model, regimes, observations, observed)))
    for key in got:
        error = float(np.abs(got[key] - want[key]).max()) if got[key].size else 0.0
        print(key, "deviation from the dense side", error)
        assert error <= EXACTNESS_TOLERANCE[key], key


# ---- 3. the degenerate models -----------------------------------------------------------------------------------------------------------
def degenerate_case(variant, seed=0):
    """(model, regimes, observations, noise) with exact zeros: 'q1' one q component 0, 'q' all q = 0 (A stays invertible:
    orthogonal times a scale), 's0' s0 = 0, 'both' s0 = 0 and q = 0 (every filtered covariance is 0)."""
    M, D, Dy, T, B, N = 2, 3, 2, 4, 2, 3
    rng = np.random.default_rng([seed, 3, 47])
    model = contract.example_model(M, D, Dy, seed=2)
    if variant == "q1":
        q = model["q"].copy()
        q[:, 1] = 0.0
        model = dict(model, q=q)
    if variant in ("q", "both"):
        model = dict(model, q=np.zeros_like(model["q"]))
    if variant in ("s0", "both"):
        model = dict(model, s0=np.zeros(D))
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    observations = [rng.standard_normal((B, Dy)) for _ in range(T)]
    noise = [rng.standard_normal((B, N, D)) for _ in range(T)]
    return model, regimes, observations, noise


def check_degenerate(variant, model, regimes, states, filtered_means, tolerances):
    """What the draws of `degenerate_case` must satisfy, whoever computed them."""
    T = len(states)
    assert all(np.isfinite(z).all() for z in states)
    if variant in ("q", "both"):      # z_{t+1} = A z_t + b exactly in real arithmetic: the draw of z_{T-1} fixes the path
        for t in range(T - 1):
            A, b = model["A"][regimes[t + 1]], model["b"][regimes[t + 1]]
            carried = np.einsum("bnij,bnj->bni", A, states[t]) + b
            allowed = np.einsum("bnij,bnj->bni", np.abs(A), tolerances[t]) + tolerances[t + 1] + \
                (model["A"].shape[-1] + 2) * contract.UNIT * (np.abs(carried) + np.abs(states[t + 1]))
            assert (np.abs(states[t + 1] - carried) <= allowed).all(), t
    if variant in ("s0", "both"):
        assert (states[0] == model["m0"]).all()
    if variant == "both":             # P = 0 with q = 0: nothing is random, every state is its filtered mean
        for t in range(T):
            assert np.array_equal(states[t], filtered_means[t])


@pytest.mark.parametrize("variant", ["q1", "q", "s0", "both"])
def test_degenerate_models_draw_without_nan_or_flag(variant):
    model, regimes, observations, noise = degenerate_case(variant)
    out = draw.state_draw_pass(model, regimes, observations, noise)
    assert out["flags"] == 0 and out["clearance"] > 1
    check_degenerate(variant, model, regimes, out["states"], out["filtered_means"], out["tolerances"]["states"])


# ---- 4. statistical ------------------------------------------------------------------------------------------------------------------------
def test_the_sample_mean_is_the_smoothed_mean():
    """One seeded pass, N = 4096: the sample mean within 5 standard errors of the smoothed mean at every t (a wrong sign is
    also caught by the exactness test; this documents the claim)."""
    M, D, Dy, T, N = 3, 2, 2, 4, 4096
    rng = np.random.default_rng(47)
    model = contract.example_model(M, D, Dy, seed=5)
    regimes = _shared_path(rng, T, 1, N, M)
    observations = [rng.standard_normal((1, Dy)) for _ in range(T)]
    out = draw.state_draw_pass(model, regimes, observations, [rng.standard_normal((1, N, D)) for _ in range(T)])
    means, covs, _ = contract.exact_state_smoother(model, [int(r[0, 0]) for r in regimes], [y[0] for y in observations])
    assert out["flags"] == 0 and out["clearance"] > 1
    for t in range(T):
        error = np.abs(out["states"][t][0].mean(axis=0) - means[t])
        assert (error <= 5 * np.sqrt(np.diagonal(covs[t]) / N)).all(), t


# ---- 5. index and time direction -----------------------------------------------------------------------------------------------------------
def test_an_out_of_range_regime_following_and_the_orientation_of_A():
    M, D, Dy, T, B, N = 3, 3, 2, 4, 2, 4
    rng = np.random.default_rng(5)
    model = contract.example_model(M, D, Dy, seed=6)
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    observations = [rng.standard_normal((B, Dy)) for _ in range(T)]
    noise = [rng.standard_normal((B, N, D)) for _ in range(T)]
    clean = draw.state_draw_pass(model, regimes, observations, noise)
    assert clean["flags"] == 0 and clean["clearance"] > 1
    # a regime outside [0, M) at step 2 is read when z_1 is drawn: NaN at steps <= 1 of that trajectory only.  (The forward
    # filter of the contract's pass meets the same regime; K47's own reading is what the step shows.)
    bad = regimes[2].copy()
    bad[1, 2] = M
    z, flags, _ = draw.state_draw_step(model, bad, clean["filtered_means"][1], clean["filtered_covariances"][1],
                                       clean["states"][2], noise[1])
    gone = np.zeros((B, N), dtype=bool)
    gone[1, 2] = True
    assert flags == draw.FLAG_INDEX_OUT_OF_RANGE and np.isnan(z[gone]).all() and np.array_equal(z[~gone], clean["states"][1][~gone])
    z0, flags, _ = draw.state_draw_step(model, regimes[1], clean["filtered_means"][0], clean["filtered_covariances"][0], z, noise[0])
    assert flags == 0 and np.isnan(z0[gone]).all() and np.array_equal(z0[~gone], clean["states"][0][~gone])
    # `following` with T = 1 is the matching step of the longer pass, bit for bit
    for t in range(T - 1):
        z, flags, _ = draw.state_draw_step(model, regimes[t + 1], clean["filtered_means"][t], clean["filtered_covariances"][t],
                                           clean["states"][t + 1], noise[t])
        assert flags == 0 and np.array_equal(z, clean["states"][t])
    chunk = draw.state_draw_pass(model, regimes[:2], observations[:2], noise[:2], following=(regimes[2], clean["states"][2]))
    assert np.array_equal(chunk["states"][1], clean["states"][1]) and np.array_equal(chunk["states"][0], clean["states"][0])
    # the orientation: A transposed moves the result far beyond the bound
    args = (regimes[3], clean["filtered_means"][2], clean["filtered_covariances"][2], clean["states"][3], noise[2])
    turned = dict(model, A=np.ascontiguousarray(np.swapaxes(model["A"], -1, -2)))
    bound, _ = draw.state_draw_step_bound(model, *args)
    moved = np.abs(draw.state_draw_step(turned, *args)[0] - draw.state_draw_step(model, *args)[0])
    assert moved.max() > 1e-3 and moved.max() > 1e6 * bound.max()
    with pytest.raises(ValueError, match="go together"):
        draw.state_draw_step(model, regimes[1], clean["filtered_means"][0], clean["filtered_covariances"][0], None, noise[0])


# ---- 6. the C entry's status codes ---------------------------------------------------------------------------------------------------------
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="non-empty sizes on made-up pointers: only where nothing can launch")
ORDER = ("model", "regimes", "mean", "cov", "noise", "regime_next", "z_next", "states", "flags", "T", "B", "N", "stream")
OPERANDS = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")


def _entry(fields=None, **changes):
    from aesmc_amd import _lib
    valid = {name: 64 * (i + 1) for i, name in enumerate(ORDER[1:9])}
    valid.update(T=3, B=0, N=3, stream=None, model=dict({key: 8 * (i + 1) for i, key in enumerate(OPERANDS)}, M=2, D=2, Dy=1))
    args = dict(valid, **changes)
    if args["model"] is not None:
        args["model"] = ctypes.byref(_lib.SwitchingModel(**dict(args["model"], **(fields or {}))))
    return _lib.load().aesmc_switching_state_draw(*[args[name] for name in ORDER])


def test_the_entry_refuses_bad_arguments_before_the_empty_launch():
    import __graft_entry__
    __graft_entry__.build()
    assert _entry() == 0 and _entry(flags=None) == 0 and _entry(regime_next=None, z_next=None) == 0
    for name in ("model", "regimes", "mean", "cov", "noise", "states"):
        assert _entry(**{name: None}) == 1, name
    assert _entry(regime_next=None) == 1 and _entry(z_next=None) == 1              # both or neither
    for name in ("A", "b", "q", "C", "d", "r"):
        assert _entry(fields={name: None}) == 1 and _entry(fields={name: 12}) == 1, name
    assert _entry(fields=dict(cdf0=None, cdf=None, m0=None, s0=None)) == 0         # (not read)
    for name in ("regimes", "regime_next", "flags"):
        assert _entry(**{name: 64 * 20 + 2}) == 1, name
    for name in ("mean", "cov", "noise", "z_next", "states"):
        assert _entry(**{name: 64 * 20 + 4}) == 1, name
    for name in ("regimes", "mean", "cov", "noise", "regime_next", "z_next"):
        assert _entry(states=64 * ORDER.index(name)) == 1, name                  # the output is an input
    assert _entry(T=0) == 1 and _entry(T=-1) == 1 and _entry(B=-1) == 1 and _entry(N=-1) == 1
    assert _entry(fields=dict(M=0)) == 1 and _entry(fields=dict(D=0)) == 1 and _entry(fields=dict(Dy=0)) == 1
    # B N == 0 is a no-op before the limits
    assert _entry(fields=dict(D=9)) == 0 and _entry(B=5, N=0, fields=dict(M=17)) == 0


@no_gpu
def test_the_entry_names_what_it_does_not_support():
    assert _entry(B=1, fields=dict(D=9)) == 2 and _entry(B=1, fields=dict(Dy=9)) == 2 and _entry(B=1, fields=dict(M=17)) == 2
    assert _entry(B=1 << 13, N=1 << 13) == 2 and _entry(B=1, N=1 << 31) == 2      # B N D^2 = 2^32 at the largest D
    assert _entry(B=1, T=0) == 1 and _entry(B=1, z_next=None) == 1                # an invalid argument comes first
    assert _entry(B=1) == 3                                                       # every check passed: the launch fails


# ---- 7. the host logic on a provider double ------------------------------------------------------------------------------------------------
class DrawOracle(OracleKernels):
    """The suite's oracle provider plus K31 (under a mask: K39) and K47 from their NumPy contracts."""

    def __init__(self):
        super().__init__()
        self.calls, self.reads, self.masks = [], 0, []

    def read_flags(self, device):
        self.reads += 1
        return super().read_flags(device)

    def switching_limits(self):
        return 8, 8, 16

    def switching_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        return torch.is_tensor(observation) and observation.dim() == 2 and observation.dtype in (torch.float32, torch.float64) \
            and observation.size(1) == observation_dim and latent_dim <= 8 and observation_dim <= 8 and num_regimes <= 16

    def switching_kalman_step(self, model, state, index, uniforms, observation, observed=None):
        self.calls.append("kalman0" if state is None else "kalman")
        self.masks.append(observed)
        ops = {name: value.numpy() for name, value in model.items()}
        parts = None if state is None else tuple(part.numpy() for part in state)
        args = (ops, parts, None, uniforms.numpy(), observation.numpy())
        regime, mean, cov, log_w, flags = contract.switching_kalman_step(*args) if observed is None else \
            missing.switching_kalman_step(*args, observed.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(log_w)

    def switching_state_draw(self, model, regimes, means, covs, noise, following=None):
        self.calls.append("draw")
        assert regimes.dtype == torch.int32 and regimes.dim() == 3 and means.dim() == covs.dim() == noise.dim() == 4
        ops = {name: value.numpy() for name, value in model.items()}
        T = means.size(0)
        regime_next, z_next = (None, None) if following is None else (following[0].numpy(), following[1].numpy())
        states = [None] * T
        for t in range(T - 1, -1, -1):
            z, flags, _ = draw.state_draw_step(ops, regime_next, means[t].numpy(), covs[t].numpy(), z_next, noise[t].numpy())
            self._flags |= flags
            states[t] = z
            regime_next, z_next = regimes[t].numpy(), z
        return torch.from_numpy(np.stack(states))


@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = DrawOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _torch_model(ops):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS])


def _host_case(T=4, B=2, N=5, M=3, D=2, Dy=2):
    rng = np.random.default_rng([T, B, N, 7])
    ops = contract.example_model(M, D, Dy, seed=5)
    model = _torch_model(ops)
    observations = model.simulate(T, B, seed=3)
    regimes = [rng.integers(0, M, (B, N)).astype(np.int32) for _ in range(T)]
    noise = [rng.standard_normal((B, N, D)) for _ in range(T)]
    return ops, model, observations, regimes, noise


def test_the_function_replays_the_contracts_pass(backend):
    from aesmc_amd import rao_blackwell
    T, B, N, D = 4, 2, 5, 2
    ops, model, observations, regimes, noise = _host_case()
    want = draw.state_draw_pass(ops, regimes, [y.numpy() for y in observations], noise)
    paths, given = [torch.from_numpy(r) for r in regimes], [torch.from_numpy(e) for e in noise]
    out = rao_blackwell.switching_sample_states(observations, model, paths, noise=given)
    assert backend.calls == ["kalman0"] + ["kalman"] * (T - 1) + ["draw"] and backend.reads == 1      # ONE launch, one read
    assert sorted(out) == ["log_likelihood", "noise", "states"]
    assert len(out["states"]) == T and all(z.shape == (B, N, D) and z.dtype == torch.float64 for z in out["states"])
    assert all(np.array_equal(z.numpy(), w) for z, w in zip(out["states"], want["states"]))
    assert np.array_equal(out["log_likelihood"].numpy(), want["log_likelihood"])
    assert all(a is b for a, b in zip(out["noise"], given))
    # views of one tensor
    base = out["states"][0]._base
    assert base is not None and all(z._base is base for z in out["states"])
    # noise=None draws it: returned, float64, of the shape, and replaying it gives the same states
    fresh = rao_blackwell.switching_sample_states(observations, model, paths)
    assert len(fresh["noise"]) == T and all(e.shape == (B, N, D) and e.dtype == torch.float64 for e in fresh["noise"])
    again = rao_blackwell.switching_sample_states(observations, model, paths, noise=fresh["noise"])
    assert all(torch.equal(a, b) for a, b in zip(fresh["states"], again["states"]))
    assert not torch.equal(fresh["states"][0], out["states"][0])
    # no gradient
    assert not out["states"][0].requires_grad


def test_noise_validation_and_the_shard_refusal(backend):
    from aesmc_amd import distributed, rao_blackwell
    ops, model, observations, regimes, noise = _host_case()
    paths, given = [torch.from_numpy(r) for r in regimes], [torch.from_numpy(e) for e in noise]
    run = lambda noise: rao_blackwell.switching_sample_states(observations, model, paths, noise=noise)
    with pytest.raises(ValueError, match="one tensor per timestep"):
        run(given[:3])
    with pytest.raises(ValueError, match="one tensor per timestep"):
        run(3.0)
    with pytest.raises(ValueError, match=r"noise\[1\] must be \(2, 5, 2\) float64"):
        run([given[0], given[1].float()] + given[2:])
    with pytest.raises(ValueError, match=r"noise\[2\]"):
        run(given[:2] + [given[2][:, :4]] + given[3:])
    with pytest.raises(ValueError, match=r"noise\[0\]"):
        run([given[0].numpy()] + given[1:])
    with pytest.raises(ValueError, match="at least one timestep"):
        rao_blackwell.switching_sample_states([], model, [])
    with pytest.raises(ValueError, match="one tensor per timestep"):
        rao_blackwell.switching_sample_states(observations, model, paths[:2])
    assert backend.calls == []
    with distributed.shard_scope(4, 0, 2):
        with pytest.raises(NotImplementedError, match="drawing the state noise inside distributed.shard_scope.*Pass noise"):
            run(None)
        assert backend.calls == []
        assert len(run(given)["states"]) == 4                                      # replayed noise is fine


def test_no_trajectories_and_one_timestep(backend):
    from aesmc_amd import rao_blackwell
    ops, model, observations, regimes, noise = _host_case()
    B, D = 2, 2
    empty = [torch.empty((B, 0), dtype=torch.int32)] * 4
    out = rao_blackwell.switching_sample_states(observations, model, empty)
    assert backend.calls == [] and backend.reads == 0                              # N == 0: nothing launched, nothing read
    assert [z.shape for z in out["states"]] == [(B, 0, D)] * 4 and out["log_likelihood"].shape == (B, 0)
    assert [e.shape for e in out["noise"]] == [(B, 0, D)] * 4
    # T == 1: the draw from the filtered law, m + chol(P) eps
    paths, given = [torch.from_numpy(regimes[0])], [torch.from_numpy(noise[0])]
    out = rao_blackwell.switching_sample_states(observations[:1], model, paths, noise=given)
    assert backend.calls == ["kalman0", "draw"]
    filtered = draw.state_draw_pass(ops, regimes[:1], [observations[0].numpy()], noise[:1])
    factor = np.linalg.cholesky(contract.unpack(filtered["filtered_covariances"][0], D))
    want = filtered["filtered_means"][0] + np.einsum("bnij,bnj->bni", factor, noise[0])
    np.testing.assert_allclose(out["states"][0].numpy(), want, rtol=0, atol=1e-14)


def test_a_regime_out_of_range_raises_once_at_the_end_and_discards_flags(backend):
    from aesmc_amd import rao_blackwell
    ops, model, observations, regimes, noise = _host_case()
    bad = [torch.from_numpy(r.copy()) for r in regimes]
    bad[2][1, 3] = 3
    given = [torch.from_numpy(e) for e in noise]
    with pytest.raises(ValueError, match="regimes holds a value outside"):
        rao_blackwell.switching_sample_states(observations, model, bad, noise=given)
    assert backend.calls == ["kalman0", "kalman", "kalman", "kalman", "draw"] and backend.reads == 1
    assert backend.read_flags(None) == 0                                           # what K31 and K47 flagged is gone
    # an exception on the way discards pending flags
    backend._flags = 4
    with pytest.raises(ValueError, match=r"noise\[0\]"):
        rao_blackwell.switching_sample_states(observations, model, bad, noise=[given[0][:1]] + given[1:])
    assert backend.read_flags(None) == 0


def test_observed_reaches_the_filter_only(backend):
    from aesmc_amd import rao_blackwell
    T = 4
    ops, model, observations, regimes, noise = _host_case()
    masks = missing.example_masks(T, 2, 2, seed=1)
    observed = [None if t == 1 else torch.from_numpy(masks[t]) for t in range(T)]
    paths, given = [torch.from_numpy(r) for r in regimes], [torch.from_numpy(e) for e in noise]
    out = rao_blackwell.switching_sample_states(observations, model, paths, noise=given, observed=observed)
    assert backend.calls == ["kalman0"] + ["kalman"] * (T - 1) + ["draw"]          # (the double's draw takes no mask at all)
    assert [m is None for m in backend.masks] == [False, True, False, False]
    want = draw.state_draw_pass(ops, regimes, [y.numpy() for y in observations], noise,
                                observed=[None if t == 1 else masks[t] for t in range(T)])
    assert all(np.array_equal(z.numpy(), w) for z, w in zip(out["states"], want["states"]))
    assert np.array_equal(out["log_likelihood"].numpy(), want["log_likelihood"])
