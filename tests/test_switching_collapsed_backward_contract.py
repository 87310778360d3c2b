"""CPU checks of the differentiable collapsed-mixture evidence of switching linear-Gaussian models (kernels K52 / K53
aesmc_switching_kalman_step_backward and its masked form, K54 aesmc_switching_collapse_backward): the NumPy contracts
(aesmc_amd/testing/switching_collapsed_backward.py) against torch.autograd of independent dense restatements, the conditioning
of every input the GPU tests use (float64 against extended precision), `collapsed_switching_log_likelihood` on a provider
double against the plain-torch restatement of the whole pass, the cases in which the gradient is that of an exact evidence,
the conventions, what the backward asks of the provider, the C entries' status codes and the refusals.

Metrics: tests/gradient_checks.py — per-slot outputs against each slot's own max|want| (a slot of scale 0 exactly zero),
per-regime and whole-pass gradients as max|diff| / max|want| without a floor; the limit is its FLOAT64_TOLERANCE."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_collapsed as collapsed
from aesmc_amd.testing import switching_collapsed_backward as backward
from tests import gradient_checks as checks
from tests.collapsed_backward_provider import CollapsedBackwardOracle

PARAMETERS = backward.PARAMETERS
LIMIT = checks.FLOAT64_TOLERANCE
CONDITION = 1e-12
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="non-empty sizes on made-up pointers: only where nothing can launch")


def slot_error(got, want):
    """(worst per-slot error, silent) of a per-slot output [B,K,..] against each slot's own max|want|."""
    got, want = torch.as_tensor(np.asarray(got, dtype=np.float64)), torch.as_tensor(np.asarray(want, dtype=np.float64))
    got, want = got.reshape(got.shape[0], got.shape[1], -1), want.reshape(want.shape[0], want.shape[1], -1)
    return checks.particle_error(got, want, want.abs().amax(dim=-1))


def reduced(got, want):
    return checks.reduced_error(torch.as_tensor(np.asarray(got, dtype=np.float64)), torch.as_tensor(np.asarray(want, dtype=np.float64)))


def assert_step_outputs(got, want, limit, what):
    for name in backward.STEP_OUTPUTS:
        if want[name] is None:
            assert got[name] is None, name
            continue
        if name in ("grad_mean_in", "grad_cov_in"):
            error, silent = slot_error(got[name], want[name])
            assert silent, (what, name)
        else:
            error = reduced(got[name], want[name])
        print(what, name, error)
        assert error <= limit, (what, name, error)


def packed_to_dense(packed, D):
    rows, cols = torch.tril_indices(D, D)
    full = packed.new_zeros(packed.shape[:-1] + (D, D))
    full[..., rows, cols] = packed
    full[..., cols, rows] = packed
    return full


def dense_to_packed(full):
    rows, cols = torch.tril_indices(full.size(-1), full.size(-1))
    return full[..., rows, cols]


def step_by_autograd(model, regime, state, y, grad_mean, grad_cov, grad_lw, observed):
    """STEP_OUTPUTS by torch.autograd of the dense restatement of one step (`backward._step`: predict, Cholesky update,
    deleted rows for the mask), the covariance entering through its PACKED vector."""
    D = model["A"].shape[-1]
    leaves = {name: torch.from_numpy(np.ascontiguousarray(model[name])).clone().requires_grad_(True)
              for name in ("m0", "s0", "A", "b", "q", "C", "d", "r")}
    B, K = regime.shape
    later = state is not None
    if later:
        mean = torch.from_numpy(state[0]).clone().requires_grad_(True)
        packed = torch.from_numpy(state[1]).clone().requires_grad_(True)
        cov = packed_to_dense(packed, D)
    else:
        mean = leaves["m0"].expand(B, K, D)
        cov = torch.diag_embed(leaves["s0"] * leaves["s0"]).expand(B, K, D, D)
    mask = None if observed is None else torch.from_numpy(observed)
    new_mean, new_cov, log_w = backward._step(mean, cov, later, leaves, torch.from_numpy(regime.astype(np.int64)),
                                              torch.from_numpy(np.asarray(y, dtype=np.float64)), mask, None)
    total = (new_mean * torch.from_numpy(grad_mean)).sum() + (dense_to_packed(new_cov) * torch.from_numpy(grad_cov)).sum() + \
        (log_w * torch.from_numpy(grad_lw)).sum()
    wanted = dict(leaves, **({"mean_in": mean, "cov_in": packed} if later else {}))
    grads = torch.autograd.grad(total, list(wanted.values()), allow_unused=True)
    out = dict.fromkeys(backward.STEP_OUTPUTS)
    for name, grad in zip(wanted, grads):
        if later and name in ("m0", "s0"):
            continue
        out["grad_" + name] = (torch.zeros_like(wanted[name]) if grad is None else grad).numpy()
    return out


# ---- 1. the contracts against torch.autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("later", [True, False])
@pytest.mark.parametrize("B,K,M,D,Dy", backward.STEP_SHAPES[:11])
def test_the_step_contract_is_autograd_of_the_dense_step(B, K, M, D, Dy, later, masked):
    args = backward.example_step_backward(B, K, M, D, Dy, later=later, masked=masked)
    got, flags = backward.switching_kalman_step_backward(*args[:7], observed=args[7])
    assert flags == 0
    assert_step_outputs(got, step_by_autograd(*args), LIMIT, "autograd")


def collapse_rows(x):
    """K54's outputs as rows of slots: a group's N log-weight gradients are one row, a component's mean or covariance
    gradient another."""
    return x.reshape(x.shape[0], -1, x.shape[-1])


def collapse_by_autograd(mean, cov, lw, grads):
    D = mean.shape[-1]
    shared = mean.ndim == 3
    leaves = [torch.from_numpy(x).clone().requires_grad_(True) for x in (mean, cov, lw)]
    G = lw.shape[1]
    m = leaves[0].unsqueeze(1).expand(-1, G, -1, -1) if shared else leaves[0]
    P = leaves[1].unsqueeze(1).expand(-1, G, -1, -1) if shared else leaves[1]
    mass, centre, spread = backward._collapse(m, packed_to_dense(P, D), leaves[2])
    total = (mass * torch.from_numpy(grads[0])).sum() + (centre * torch.from_numpy(grads[1])).sum() + \
        (dense_to_packed(spread) * torch.from_numpy(grads[2])).sum()
    g_mean, g_cov, g_lw = torch.autograd.grad(total, leaves)
    return g_lw.numpy(), g_mean.numpy(), g_cov.numpy()


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,G,N,D", collapsed.COLLAPSE_SHAPES[:4])
def test_the_collapse_contract_is_autograd_of_the_mixtures_moments(B, G, N, D, shared):
    mean, cov, lw = collapsed.example_collapse(B, G, N, D)
    if shared:
        mean, cov = np.ascontiguousarray(mean[:, 0]), np.ascontiguousarray(cov[:, 0])
    grads = backward.example_collapse_backward(B, G, N, D)
    got = backward.switching_collapse_backward(mean, cov, lw, *grads)
    want = collapse_by_autograd(mean, cov, lw, grads)
    for name, value, reference in zip(("log_weight", "mean", "cov"), got, want):
        assert value.shape == reference.shape
        error, silent = slot_error(collapse_rows(value), collapse_rows(reference))
        print(name, error)
        assert silent and error <= LIMIT, name


# ---- 2. conditioning: float64 against extended precision on every input of the GPU tests -------------------------------------------------
@pytest.mark.parametrize("y_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("later", [True, False])
@pytest.mark.parametrize("B,K,M,D,Dy", backward.STEP_SHAPES)
def test_the_step_inputs_are_well_conditioned(B, K, M, D, Dy, later, masked, y_dtype):
    args = backward.example_step_backward(B, K, M, D, Dy, later=later, masked=masked, observation_dtype=y_dtype)
    got, _ = backward.switching_kalman_step_backward(*args[:7], observed=args[7])
    wide, _ = backward.switching_kalman_step_backward(*args[:7], observed=args[7], dtype=np.longdouble)
    assert_step_outputs(got, wide, CONDITION, "extended")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,G,N,D", collapsed.COLLAPSE_SHAPES)
def test_the_collapse_inputs_are_well_conditioned(B, G, N, D, shared):
    mean, cov, lw = collapsed.example_collapse(B, G, N, D)
    if shared:
        mean, cov = mean[:, 0], cov[:, 0]
    grads = backward.example_collapse_backward(B, G, N, D)
    got = backward.switching_collapse_backward(mean, cov, lw, *grads)
    wide = backward.switching_collapse_backward(mean, cov, lw, *grads, dtype=np.longdouble)
    for name, value, reference in zip(("log_weight", "mean", "cov"), got, wide):
        error, silent = slot_error(collapse_rows(value), collapse_rows(reference))
        print(name, error)
        assert silent and error <= CONDITION, name


# ---- 3. the whole pass on a provider double ------------------------------------------------------------------------------------------------
@pytest.fixture
def backend():
    from aesmc_amd import _kernels
    provider = CollapsedBackwardOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def leaves_of(ops, shared=()):
    """The ten parameters as leaves that require grad; `shared`: names given with a leading 1 (regime 0's for all)."""
    out = {}
    for name in PARAMETERS:
        value = torch.from_numpy(np.ascontiguousarray(ops[name][:1] if name in shared else ops[name])).clone()
        out[name] = value.requires_grad_(True)
    return out


def share(ops, names):
    out = dict(ops)
    for name in names:
        out[name] = np.ascontiguousarray(np.broadcast_to(ops[name][:1], ops[name].shape))
    return out


def observations_of(ops, T, B, seed=0):
    rng = np.random.default_rng([seed, T, B, 5253])
    return [torch.from_numpy(rng.standard_normal((B, ops["C"].shape[-2]))) for _ in range(T)]


def both_gradients(observations, ops, order, observed=None, shared=()):
    from aesmc_amd import rao_blackwell
    mine, theirs = leaves_of(ops, shared), leaves_of(ops, shared)
    value = rao_blackwell.collapsed_switching_log_likelihood(observations, mine, order=order, observed=observed)
    want = backward.collapsed_log_likelihood_restated(observations, theirs, order=order, observed=observed)
    weights = torch.linspace(0.5, 1.5, value.numel(), dtype=torch.float64)
    got_grads = torch.autograd.grad((value * weights).sum(), list(mine.values()), allow_unused=True)
    want_grads = torch.autograd.grad((want * weights).sum(), list(theirs.values()), allow_unused=True)
    # (a parameter the pass does not read — Pi at T == 1 — has gradient zero on both sides)
    fill = lambda grads, leaves: {name: torch.zeros_like(leaves[name]) if grad is None else grad
                                  for name, grad in zip(PARAMETERS, grads)}
    return value, want, fill(got_grads, mine), fill(want_grads, theirs)


def assert_gradients(got, want, limit=LIMIT):
    for name in PARAMETERS:
        assert got[name] is not None and want[name] is not None, name
        error = checks.reduced_error(got[name], want[name])
        print(name, error)
        assert error <= limit, (name, error)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("M,D,Dy", [(2, 2, 1), (3, 3, 2), (4, 2, 2)])
def test_the_pass_and_its_gradients_are_the_restatements(backend, M, D, Dy, T, order):
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(M, D, Dy)
    observations = observations_of(ops, T, 3)
    value, want, got_grads, want_grads = both_gradients(observations, ops, order)
    assert value.shape == (3,) and value.dtype == torch.float64 and value.requires_grad
    assert float((value - want).detach().abs().max()) <= 1e-12 * (1 + float(want.detach().abs().max()))
    assert_gradients(got_grads, want_grads)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in PARAMETERS])
    filtered = rao_blackwell.collapsed_switching_filter(observations, model, order=order)["log_marginal_likelihood"]
    assert torch.equal(value.detach(), filtered)
    plain = rao_blackwell.collapsed_switching_log_likelihood(observations, model, order=order)
    assert torch.equal(plain, filtered) and not plain.requires_grad
    loss = rao_blackwell.collapsed_switching_loss(observations, leaves_of(ops), order=order)
    assert loss.dim() == 0 and torch.equal(loss.detach(), -filtered.mean())


@pytest.mark.parametrize("order", [2, 1])
def test_a_masked_pass_and_a_shared_parameter(backend, order):
    from aesmc_amd import rao_blackwell
    from aesmc_amd.testing import switching_missing as missing
    T, B = 4, 3
    ops = share(contract.example_model(3, 3, 2), ("C", "r"))
    observations = observations_of(ops, T, B)
    masks = missing.example_masks(T, B, 2, seed=1)
    observed = [None if t == 1 else torch.from_numpy(masks[t]) for t in range(T)]
    hidden = [y if observed[t] is None else torch.where(observed[t], y, torch.full_like(y, float("nan")))
              for t, y in enumerate(observations)]
    value, want, got_grads, want_grads = both_gradients(hidden, ops, order, observed=observed, shared=("C", "r"))
    assert float((value - want).detach().abs().max()) <= 1e-12 * (1 + float(want.detach().abs().max()))
    assert got_grads["C"].shape == (1, 2, 3) and got_grads["r"].shape == (1, 2)
    assert_gradients(got_grads, want_grads)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in PARAMETERS])
    for series in (hidden, [y.float() for y in hidden]):
        filtered = rao_blackwell.collapsed_switching_filter(series, model, order=order, observed=observed)
        again = rao_blackwell.collapsed_switching_log_likelihood(series, leaves_of(ops), order=order, observed=observed)
        assert torch.equal(again.detach(), filtered["log_marginal_likelihood"])
    assert any(mask for (_, _, _, mask) in [a for a in backend.asked if a[0].startswith("kalman")])


# ---- 4. exactness: the gradient of something that is not an approximation ----------------------------------------------------------------
def kalman_log_likelihood(observations, p):
    """log p(y) [B] of the one-regime model by a plain torch Kalman filter (explicit inverse, no Cholesky)."""
    A, b, q, C, d, r = (p[name][0] for name in ("A", "b", "q", "C", "d", "r"))
    B, Dy = observations[0].shape
    mean = p["m0"].expand(B, -1)
    cov = torch.diag(p["s0"].reshape(-1).expand(A.size(0)) ** 2)
    total = 0.0
    for t, y in enumerate(observations):
        if t > 0:
            mean, cov = mean @ A.t() + b, A @ cov @ A.t() + torch.diag(q * q)
        S = C @ cov @ C.t() + torch.diag(r * r)
        e = y - mean @ C.t() - d
        inverse = torch.linalg.inv(S)
        total = total - 0.5 * ((e @ inverse) * e).sum(-1) - 0.5 * torch.logdet(S) - Dy * contract.HALF_LOG_2PI
        gain = cov @ C.t() @ inverse
        mean, cov = mean + e @ gain.t(), cov - gain @ C @ cov
    return total


def enumerated_log_likelihood(observations, p):
    """log p(y) [B] by enumerating all M^T regime paths, each a plain torch Kalman filter."""
    M, T = p["pi0"].numel(), len(observations)
    terms = []
    for path in itertools.product(range(M), repeat=T):
        one = {name: p[name] for name in ("m0", "s0")}
        prior = torch.log(p["pi0"][path[0]])
        B, Dy = observations[0].shape
        mean = p["m0"].expand(B, -1)
        cov = torch.diag(p["s0"] ** 2)
        total = prior
        for t, s in enumerate(path):
            A, b, q, C, d, r = (p[name][s] for name in ("A", "b", "q", "C", "d", "r"))
            if t > 0:
                total = total + torch.log(p["Pi"][path[t - 1], s])
                mean, cov = mean @ A.t() + b, A @ cov @ A.t() + torch.diag(q * q)
            S = C @ cov @ C.t() + torch.diag(r * r)
            e = observations[t] - mean @ C.t() - d
            inverse = torch.linalg.inv(S)
            total = total - 0.5 * ((e @ inverse) * e).sum(-1) - 0.5 * torch.logdet(S) - Dy * contract.HALF_LOG_2PI
            gain = cov @ C.t() @ inverse
            mean, cov = mean + e @ gain.t(), cov - gain @ C @ cov
        terms.append(total)
        del one
    return torch.logsumexp(torch.stack(terms), dim=0)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("T", [1, 3, 5])
def test_one_regime_gives_the_kalman_filters_gradients(backend, T, order):
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(1, 3, 2, seed=2)
    observations = observations_of(ops, T, 2)
    mine, theirs = leaves_of(ops), leaves_of(ops)
    value = rao_blackwell.collapsed_switching_log_likelihood(observations, mine, order=order)
    want = kalman_log_likelihood(observations, theirs)
    assert float((value - want).detach().abs().max()) <= 1e-12 * (1 + float(want.detach().abs().max()))
    names = [name for name in PARAMETERS if name not in ("pi0", "Pi")]      # (one regime: the chain has no free parameter)
    got = torch.autograd.grad(value.sum(), [mine[name] for name in names], allow_unused=True)
    ref = torch.autograd.grad(want.sum(), [theirs[name] for name in names], allow_unused=True)
    for name, g, w in zip(names, got, ref):
        if w is None:      # (T == 1: the dynamics are not read)
            assert g is None or float(g.abs().max()) == 0.0, name
            continue
        error = checks.reduced_error(g, w)
        print(name, error)
        assert error <= LIMIT, name


def test_order_two_at_two_steps_gives_the_enumerations_gradients(backend):
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(2, 2, 2, seed=1)
    observations = observations_of(ops, 2, 3)
    mine, theirs = leaves_of(ops), leaves_of(ops)
    value = rao_blackwell.collapsed_switching_log_likelihood(observations, mine, order=2)
    want = enumerated_log_likelihood(observations, theirs)
    assert float((value - want).detach().abs().max()) <= 1e-12 * (1 + float(want.detach().abs().max()))
    got = torch.autograd.grad(value.sum(), list(mine.values()))
    ref = torch.autograd.grad(want.sum(), list(theirs.values()))
    assert_gradients(dict(zip(PARAMETERS, got)), dict(zip(PARAMETERS, ref)))


# ---- 5. the conventions ------------------------------------------------------------------------------------------------------------------------
def test_structural_zeros_give_zero_gradients_and_finite_others(backend):
    """Pi[0,1] = 0 and pi0[1] = 0 exactly, and regime 1's innovation covariance singular at step 0 (C_1 = 0, r_1 = 0: its
    step-0 forward is NaN), where only the excluded regime meets it."""
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(2, 2, 1, seed=3)
    Pi = np.array([[1.0, 0.0], [0.4, 0.6]])
    pi0 = np.array([1.0, 0.0])
    ops = contract.operands(pi0, Pi, ops["m0"], ops["s0"], ops["A"], ops["b"], ops["q"], ops["C"], ops["d"], ops["r"])
    observations = observations_of(ops, 3, 2)
    value, want, got, ref = both_gradients(observations, ops, 2)
    assert bool(torch.isfinite(value).all())
    assert float(got["Pi"][0, 1]) == 0.0 and float(got["pi0"][1]) == 0.0
    for name in PARAMETERS:
        assert bool(torch.isfinite(got[name]).all()), name
    assert_gradients(got, ref)
    # a singular innovation under the excluded regime: the forward of that slot is NaN, its arriving gradient zero
    singular = dict(ops, C=ops["C"].copy(), r=ops["r"].copy())
    singular["C"][1], singular["r"][1] = 0.0, 0.0
    leaves = leaves_of(singular)
    out = rao_blackwell.collapsed_switching_log_likelihood(observations[:1], leaves, order=2)
    grads = torch.autograd.grad(out.sum(), list(leaves.values()), allow_unused=True)
    for name, grad in zip(PARAMETERS, grads):
        assert (grad is None and name == "Pi") or bool(torch.isfinite(grad).all()), name      # (T == 1 does not read Pi)
    assert float(grads[0][1]) == 0.0 and float(grads[PARAMETERS.index("C")][1].abs().max()) == 0.0


def test_dead_components_empty_groups_and_nan_weights():
    mean, cov, lw = collapsed.example_collapse(2, 3, 4, 2)
    grads = backward.example_collapse_backward(2, 3, 4, 2)
    lw[0, 0, 1] = -np.inf
    mean[0, 0, 1], cov[0, 0, 1] = np.nan, np.nan      # a dead component is not read
    lw[0, 1, :] = -np.inf                             # an empty group
    lw[1, 2, 0] = np.nan                              # a NaN weight
    g_lw, g_mean, g_cov = backward.switching_collapse_backward(mean, cov, lw, *grads)
    assert g_lw[0, 0, 1] == 0.0 and (g_mean[0, 0, 1] == 0.0).all() and (g_cov[0, 0, 1] == 0.0).all()
    assert np.isfinite(g_lw[0, 0]).all() and np.isfinite(g_mean[0, 0]).all()
    assert (g_lw[0, 1] == 0.0).all() and (g_mean[0, 1] == 0.0).all() and (g_cov[0, 1] == 0.0).all()
    assert np.isnan(g_lw[1, 2]).all() and np.isnan(g_mean[1, 2]).all() and np.isnan(g_cov[1, 2]).all()
    assert np.isfinite(g_lw[1, :2]).all() and np.isfinite(g_lw[0, 2]).all()
    # the live components of group (0,0) are those of the group without the dead one
    keep = [0, 2, 3]
    alone = backward.switching_collapse_backward(mean[:1, :1, keep], cov[:1, :1, keep], lw[:1, :1, keep],
                                                 grads[0][:1, :1], grads[1][:1, :1], grads[2][:1, :1])
    assert np.abs(alone[0][0, 0] - g_lw[0, 0, keep]).max() <= 1e-14 and np.abs(alone[1][0, 0] - g_mean[0, 0, keep]).max() <= 1e-14


def test_a_silent_slot_writes_zeros_whatever_its_forward_is():
    args = list(backward.example_step_backward(2, 4, 2, 2, 1))
    model = dict(args[0], C=args[0]["C"].copy(), r=args[0]["r"].copy())
    model["C"][1], model["r"][1] = 0.0, 0.0           # regime 1: S = 0, the forward is NaN
    regime = args[1].copy()
    regime[:, :] = 0
    regime[0, 2] = 1
    for grad in args[4:7]:
        grad[0, 2] = 0.0
    out, flags = backward.switching_kalman_step_backward(model, regime, *args[2:7])
    assert flags == 0
    assert (out["grad_mean_in"][0, 2] == 0.0).all() and (out["grad_cov_in"][0, 2] == 0.0).all()
    for name in backward.STEP_OUTPUTS:
        if out[name] is not None:
            assert np.isfinite(out[name]).all(), name
    assert (out["grad_C"][1] == 0.0).all() and (out["grad_A"][1] == 0.0).all()
    # with a gradient arriving, the same slot is NaN; a regime outside [0, M) raises the flag and adds nothing
    args[6][0, 2] = 1.0
    out, _ = backward.switching_kalman_step_backward(model, regime, *args[2:7])
    assert np.isnan(out["grad_mean_in"][0, 2]).all() and np.isnan(out["grad_C"][1]).all() and np.isfinite(out["grad_C"][0]).all()
    regime[0, 2] = 2
    out, flags = backward.switching_kalman_step_backward(model, regime, *args[2:7])
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE and np.isnan(out["grad_cov_in"][0, 2]).all()
    assert np.isfinite(out["grad_C"]).all() and (out["grad_C"][1] == 0.0).all()


# ---- 6. what the backward asks of the provider ------------------------------------------------------------------------------------------------
def test_only_what_needs_a_gradient_is_asked_for(backend):
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(2, 2, 2)
    observations = observations_of(ops, 3, 2)
    leaves = {name: torch.from_numpy(ops[name].copy()) for name in PARAMETERS}
    leaves["C"].requires_grad_(True)
    value = rao_blackwell.collapsed_switching_log_likelihood(observations, leaves, order=2)
    assert backend.asked == [] and backend.reads == 1
    (grad,) = torch.autograd.grad(value.sum(), [leaves["C"]])
    assert grad.shape == (2, 2, 2) and backend.reads == 1
    steps = [a for a in backend.asked if a[0].startswith("kalman")]
    assert [a[0] for a in steps] == ["kalman", "kalman", "kalman0"]
    assert all(a[2] == ("C",) for a in steps) and [a[1] for a in steps] == [True, True, False]
    merges = [a for a in backend.asked if a[0] == "collapse"]
    assert len(merges) == 5 and all(a[1] == "dense" for a in merges)
    with pytest.raises(RuntimeError):      # first order only
        value = rao_blackwell.collapsed_switching_log_likelihood(observations, leaves, order=2)
        (grad,) = torch.autograd.grad(value.sum(), [leaves["C"]], create_graph=True)
        grad.sum().backward()


# ---- 7. the C entries' status codes --------------------------------------------------------------------------------------------------------------
STEP_ORDER = ("y_dtype", "model", "regime", "mean_in", "cov_in", "y", "grad_mean", "grad_cov", "grad_log_weight", "grad_mean_in",
              "grad_cov_in", "grad_m0", "grad_s0", "grad_A", "grad_b", "grad_q", "grad_C", "grad_d", "grad_r", "workspace",
              "workspace_bytes", "flags", "B", "K", "stream")
MASKED_ORDER = STEP_ORDER[:6] + ("observed",) + STEP_ORDER[6:]
OPERANDS = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
BIG = 0x7fffffff


def _step_entry(masked=False, fields=None, **changes):
    """The status of a later step's call on made-up pointers (distinct multiples of 64), B = 0 unless changed."""
    from aesmc_amd import _lib
    order = MASKED_ORDER if masked else STEP_ORDER
    args = {name: 64 * (i + 1) for i, name in enumerate(order)}
    args.update(y_dtype=_lib.F64, grad_m0=None, grad_s0=None, workspace_bytes=1 << 40, B=0, K=3, stream=None)
    args["model"] = dict({key: 8192 + 64 * i for i, key in enumerate(OPERANDS)}, M=2, D=2, Dy=1)
    args.update(changes)
    if args["model"] is not None:
        args["model"] = ctypes.byref(_lib.SwitchingModel(**dict(args["model"], **(fields or {}))))
    name = "aesmc_switching_kalman_masked_step_backward" if masked else "aesmc_switching_kalman_step_backward"
    return getattr(_lib.load(), name)(*[args[name_] for name_ in order])


@pytest.mark.parametrize("masked", [False, True])
def test_the_step_backward_entry_refuses_bad_arguments_before_the_empty_launch(masked):
    import __graft_entry__
    __graft_entry__.build()
    entry = lambda **changes: _step_entry(masked, **changes)
    outputs = ("grad_mean_in", "grad_cov_in", "grad_A", "grad_b", "grad_q", "grad_C", "grad_d", "grad_r")
    assert entry() == 0 and entry(B=2, K=0) == 0 and entry(B=-1) == 1 and entry(K=-1) == 1
    for name in ("model", "regime", "y", "grad_mean", "grad_cov", "grad_log_weight"):
        assert entry(**{name: None}) == 1, name
    assert entry(mean_in=None) == 1 and entry(cov_in=None) == 1                     # the stored two come together
    assert entry(**{name: None for name in outputs}) == 1                          # nothing asked for
    assert entry(flags=None) == 0 and entry(**{name: None for name in outputs[1:]}) == 0
    assert entry(grad_m0=4096) == 1 and entry(grad_s0=4096) == 1                    # a later step does not read the initial state
    step0 = dict(mean_in=None, cov_in=None, grad_mean_in=None, grad_cov_in=None)
    assert entry(**step0) == 0 and entry(**dict(step0, grad_m0=4096, grad_s0=4160)) == 0
    assert entry(**dict(step0, grad_mean_in=64 * 10)) == 1 and entry(**dict(step0, grad_cov_in=64 * 11)) == 1
    for name in ("regime", "mean_in", "cov_in", "grad_mean", "grad_cov", "grad_log_weight", "workspace", "flags") + outputs:
        assert entry(**{name: 64 * 40 + (2 if name in ("regime", "flags") else 4)}) == 1, name
    assert entry(y=4) == 1 and entry(y=4, y_dtype=0) == 0 and entry(y_dtype=2) == 1
    for key in OPERANDS[2:]:
        assert entry(fields={key: None}) == 1 and entry(fields={key: 4}) == 1, key
    assert entry(fields=dict(cdf0=None, cdf=None)) == 0                             # the chain's rows are not read
    for field in ("M", "D", "Dy"):
        assert entry(fields={field: 0}) == 1
    order = MASKED_ORDER if masked else STEP_ORDER
    inputs = ("regime", "mean_in", "cov_in", "y", "grad_mean", "grad_cov", "grad_log_weight") + (("observed",) if masked else ())
    for i, out in enumerate(outputs + ("workspace",)):
        for source in inputs + (outputs + ("workspace",))[:i]:
            assert entry(**{out: 64 * (order.index(source) + 1)}) == 1, (out, source)
        assert entry(**{out: 8192 + 64 * 4}) == 1, out                              # the model's A
    assert entry(workspace=None) == 4 and entry(workspace=None, **{name: None for name in outputs[2:]}) == 0
    if masked:
        assert entry(observed=None) == 1 and entry(observed=64 * 7 + 1) == 0
    # B K == 0 is a no-op before the limits; an invalid argument beside an unsupported extent is invalid
    assert entry(fields=dict(D=9)) == 0 and entry(fields=dict(M=17), B=2, K=0) == 0
    assert entry(fields=dict(D=9), regime=None) == 1 and entry(fields=dict(Dy=9, A=None)) == 1


@no_gpu
@pytest.mark.parametrize("masked", [False, True])
def test_the_step_backward_entry_names_what_it_does_not_support(masked):
    from aesmc_amd import _lib
    entry = lambda **changes: _step_entry(masked, **changes)
    for extent in (dict(D=9), dict(Dy=9), dict(M=17)):
        assert entry(B=2, fields=extent) == 2, extent
    assert entry(B=BIG + 1, K=1) == 2 and entry(B=1, K=BIG + 1) == 2 and entry(B=1 << 16, K=1 << 16) == 2
    assert entry(B=2, workspace_bytes=(2 * 3 + 64 * 16) * 16 * 8 - 1) == 4 and entry(B=2, workspace_bytes=(2 * 3 + 64 * 16) * 16 * 8) == 3
    assert entry(B=2) == 3
    lib = _lib.load()
    assert lib.aesmc_switching_backward_workspace_bytes(2, 3, 2, 1) == (2 * 3 + 64 * 16) * (4 + 4 + 2 + 2 + 4) * 8      # the slots' rows, then the parts' sums
    assert lib.aesmc_switching_backward_workspace_bytes(0, 3, 2, 1) == 0 and lib.aesmc_switching_backward_workspace_bytes(1, 1, 9, 1) == 0


COLLAPSE_ORDER = ("mean", "mean_stride", "cov", "cov_stride", "log_weight", "grad_log_mass", "grad_mean_out", "grad_cov_out",
                  "grad_log_weight", "grad_mean", "grad_cov", "B", "G", "N", "D", "stream")


def _collapse_entry(**changes):
    from aesmc_amd import _lib
    args = {name: 64 * (i + 1) for i, name in enumerate(COLLAPSE_ORDER)}
    args.update(B=0, G=2, N=3, D=2, mean_stride=6, cov_stride=9, stream=None)
    args.update(changes)
    return _lib.load().aesmc_switching_collapse_backward(*[args[name] for name in COLLAPSE_ORDER])


def test_the_collapse_backward_entry_refuses_bad_arguments_before_the_empty_launch():
    import __graft_entry__
    __graft_entry__.build()
    assert _collapse_entry() == 0 and _collapse_entry(B=2, G=0) == 0
    pointers = [name for name in COLLAPSE_ORDER[:11] if not name.endswith("stride")]
    outputs = ("grad_log_weight", "grad_mean", "grad_cov")
    for name in pointers:
        assert _collapse_entry(**{name: None}) == (0 if name in outputs else 1), name
        assert _collapse_entry(**{name: 64 * 30 + 4}) == 1, name
    assert _collapse_entry(**{name: None for name in outputs}) == 1
    assert _collapse_entry(B=-1) == 1 and _collapse_entry(G=-1) == 1 and _collapse_entry(N=-1) == 1 and _collapse_entry(D=0) == 1
    assert _collapse_entry(mean_stride=5) == 1 and _collapse_entry(cov_stride=8) == 1
    assert _collapse_entry(mean_stride=0, cov_stride=0) == 0 and _collapse_entry(mean_stride=0) == 1      # shared together
    for i, out in enumerate(outputs):
        for source in tuple(pointers[:6]) + outputs[:i]:
            assert _collapse_entry(**{out: 64 * (COLLAPSE_ORDER.index(source) + 1)}) == 1, (out, source)
    assert _collapse_entry(D=9, mean_stride=27, cov_stride=135) == 0 and _collapse_entry(D=9, mean_stride=27, cov_stride=135, mean=None) == 1


@no_gpu
def test_the_collapse_backward_entry_names_what_it_does_not_support():
    assert _collapse_entry(B=1, D=9, mean_stride=27, cov_stride=135) == 2
    assert _collapse_entry(B=1, N=257, mean_stride=514, cov_stride=771) == 2 and _collapse_entry(B=1, G=257) == 2
    assert _collapse_entry(B=BIG + 1, G=1) == 2
    assert _collapse_entry(B=1) == 3 and _collapse_entry(B=1, mean_stride=0, cov_stride=0) == 3


# ---- 8. the refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal(backend, monkeypatch):
    from aesmc_amd import distributed, rao_blackwell
    ops = contract.example_model(2, 2, 2)
    observations = observations_of(ops, 3, 2)
    leaves = leaves_of(ops)
    run = rao_blackwell.collapsed_switching_log_likelihood
    for order in (0, 3, "2", None):
        with pytest.raises(ValueError, match="order must be 1 or 2"):
            run(observations, leaves, order=order)
    with pytest.raises(ValueError, match="at least one timestep"):
        run([], leaves)
    with pytest.raises(ValueError, match="mapping with the keys"):
        run(observations, {name: leaves[name] for name in PARAMETERS[:-1]})
    with pytest.raises(ValueError, match="must be a float64 tensor"):
        run(observations, dict(leaves, A=leaves["A"].detach().float()))
    with pytest.raises(ValueError, match="must sum to 1"):
        run(observations, dict(leaves, Pi=leaves["Pi"].detach() * 0.5))
    with pytest.raises(ValueError, match="observed must be None or hold one entry per timestep"):
        run(observations, leaves, observed=[None])
    with pytest.raises(NotImplementedError, match="these observations"):
        run([y.to(torch.float16) for y in observations], leaves)
    assert backend.calls == [] and backend.reads == 0
    monkeypatch.setattr(distributed, "active_shard", lambda: object())
    with pytest.raises(NotImplementedError, match="shard_scope"):
        run(observations, leaves)
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="hipGraph"):
        run(observations, leaves)
    monkeypatch.undo()
    assert backend.calls == [] and backend.reads == 0
    poisoned = [observations[0], torch.full_like(observations[1], float("nan")), observations[2]]
    with pytest.raises(FloatingPointError, match="nan"):
        run(poisoned, leaves)
    assert backend.reads == 1
