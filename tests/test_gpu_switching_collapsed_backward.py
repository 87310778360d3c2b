"""The differentiable collapsed-mixture evidence of switching linear-Gaussian models on the device: kernels K52 / K53
(aesmc_switching_kalman_step_backward and its masked form) and K54 (aesmc_switching_collapse_backward) against their NumPy
contracts (aesmc_amd/testing/switching_collapsed_backward.py), their conventions, bit-equal repeats, and
`aesmc_amd.rao_blackwell.collapsed_switching_log_likelihood` end to end: its value `torch.equal` to the filter's and its ten
gradients against the plain-torch restatement of the whole pass on the CPU.

Metrics and limit: tests/gradient_checks.py — per-slot outputs against each slot's own max|want| (a slot of scale 0 exactly
zero), per-regime and whole-pass gradients as max|diff| / max|want| without a floor, FLOAT64_TOLERANCE.  That no input here
can hide or invent a failure under that limit is asserted by the CPU suite (float64 against extended precision within 1e-12
on every input: tests/test_switching_collapsed_backward_contract.py)."""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_collapsed as collapsed
from aesmc_amd.testing import switching_collapsed_backward as backward
from aesmc_amd.testing import switching_missing as missing
from tests import gradient_checks as checks
from tests.test_switching_collapsed_backward_contract import (PARAMETERS, assert_gradients, collapse_rows, leaves_of,
                                                              observations_of, slot_error, reduced)

pytestmark = pytest.mark.gpu

LIMIT = checks.FLOAT64_TOLERANCE
GRADIENTS = ("m0", "s0", "A", "b", "q", "C", "d", "r")


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device):
    return None if array is None else torch.from_numpy(np.array(array)).to(device)


def _device_step(provider, device, args, need_state, need):
    model, regime, state, y, grad_mean, grad_cov, grad_lw, observed = args
    ops = {name: _dev(value, device) for name, value in model.items()}
    parts = None if state is None else tuple(_dev(part, device) for part in state)
    return provider.switching_kalman_step_backward(ops, _dev(regime, device), parts, _dev(y, device), _dev(grad_mean, device),
                                                   _dev(grad_cov, device), _dev(grad_lw, device), observed=_dev(observed, device),
                                                   need_state=need_state, need=need)


# ---- K52 / K53 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("later", [True, False])
@pytest.mark.parametrize("B,K,M,D,Dy", backward.STEP_SHAPES)
def test_the_step_backward_equals_the_contract(hip_device, B, K, M, D, Dy, later, masked, y_dtype):
    provider = _provider()
    args = backward.example_step_backward(B, K, M, D, Dy, later=later, masked=masked, observation_dtype=y_dtype)
    want, _ = backward.switching_kalman_step_backward(*args[:7], observed=args[7])
    names = tuple(name for name in GRADIENTS if want["grad_" + name] is not None)
    # everything in one launch, and a repeat
    mean_in, cov_in, grads = _device_step(provider, hip_device, args, later, names)
    again = _device_step(provider, hip_device, args, later, names)
    assert provider.read_flags(hip_device) == 0
    got = dict({"grad_" + name: grads[name].cpu().numpy() for name in names},
               grad_mean_in=None if mean_in is None else mean_in.cpu().numpy(),
               grad_cov_in=None if cov_in is None else cov_in.cpu().numpy())
    worst = 0.0
    for name in backward.STEP_OUTPUTS:
        if want[name] is None:
            assert got.get(name) is None, name
            continue
        assert got[name].shape == want[name].shape and got[name].dtype == np.float64, name
        if name in ("grad_mean_in", "grad_cov_in"):
            error, silent = slot_error(got[name], want[name])
            assert silent, name
        else:
            error = reduced(got[name], want[name])
        worst = max(worst, error)
        assert error <= LIMIT, (name, error)
    print("largest error", worst)
    if later:
        assert torch.equal(mean_in, again[0]) and torch.equal(cov_in, again[1])
    for name in names:
        assert torch.equal(grads[name], again[2][name]), name      # no atomics, one order: the same bits
    # each output alone, the others NULL: the same bits as together
    if later:
        alone = _device_step(provider, hip_device, args, True, ())
        assert alone[2] == {} and torch.equal(alone[0], mean_in) and torch.equal(alone[1], cov_in)
        only_mean = _device_step(provider, hip_device, args, (True, False), ())
        only_cov = _device_step(provider, hip_device, args, (False, True), ())
        assert only_mean[1] is None and only_cov[0] is None and only_mean[2] == {} and only_cov[2] == {}
        assert torch.equal(only_mean[0], mean_in) and torch.equal(only_cov[1], cov_in)
    for name in names:
        alone = _device_step(provider, hip_device, args, False, (name,))
        assert alone[0] is None and alone[1] is None and list(alone[2]) == [name]
        assert torch.equal(alone[2][name], grads[name]), name


def test_the_step_backwards_conventions_on_the_device(hip_device):
    provider = _provider()
    args = list(backward.example_step_backward(2, 4, 2, 2, 1))
    model = dict(args[0], C=args[0]["C"].copy(), r=args[0]["r"].copy())
    model["C"][1], model["r"][1] = 0.0, 0.0           # regime 1: S = 0, the forward is NaN
    regime = args[1].copy()
    regime[:, :] = 0
    regime[0, 2] = 1
    for grad in args[4:7]:
        grad[0, 2] = 0.0
    case = [model, regime] + args[2:]
    mean_in, cov_in, grads = _device_step(provider, hip_device, case, True, GRADIENTS[2:])
    assert provider.read_flags(hip_device) == 0
    want, _ = backward.switching_kalman_step_backward(*case[:7])
    assert bool((mean_in[0, 2] == 0).all()) and bool((cov_in[0, 2] == 0).all())
    assert bool(torch.isfinite(mean_in).all()) and bool(torch.isfinite(cov_in).all())
    for name in GRADIENTS[2:]:
        assert bool(torch.isfinite(grads[name]).all()), name
        assert reduced(grads[name].cpu().numpy(), want["grad_" + name]) <= LIMIT, name
    assert bool((grads["C"][1] == 0).all()) and bool((grads["A"][1] == 0).all())
    # a regime outside [0, M): the flag, NaN rows, nothing added to any sum
    regime[0, 2] = 2
    case[4][0, 2] = 1.0
    mean_in, cov_in, grads = _device_step(provider, hip_device, case, True, GRADIENTS[2:])
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    want, flags = backward.switching_kalman_step_backward(*case[:7])
    assert flags == contract.FLAG_INDEX_OUT_OF_RANGE
    assert bool(torch.isnan(mean_in[0, 2]).all()) and bool(torch.isnan(cov_in[0, 2]).all())
    assert int(torch.isnan(mean_in).sum()) == 2 and bool(torch.isfinite(grads["C"]).all())
    for name in GRADIENTS[2:]:
        assert reduced(grads[name].cpu().numpy(), want["grad_" + name]) <= LIMIT, name
    # a masked row: a deleted component adds exactly nothing to C, d and r, and its y (NaN) reaches nothing
    args = list(backward.example_step_backward(2, 4, 2, 2, 3, masked=True))
    args[7][:] = np.array([[True, False, True], [False, False, True]])
    args[3] = np.where(args[7], np.nan_to_num(args[3]), np.nan)
    args[1][:] = np.array([[0, 0, 0, 0], [1, 1, 1, 1]])
    _, _, grads = _device_step(provider, hip_device, args, True, GRADIENTS[2:])
    assert provider.read_flags(hip_device) == 0
    assert bool((grads["C"][:, 1] == 0).all()) and bool((grads["d"][:, 1] == 0).all()) and bool((grads["r"][:, 1] == 0).all())
    assert bool((grads["C"][1, 0] == 0).all()) and bool((grads["r"][1, 0] == 0).all()) and bool((grads["r"][0, 0] != 0).all())
    for name in GRADIENTS[2:]:
        assert bool(torch.isfinite(grads[name]).all()), name


# ---- K54 --------------------------------------------------------------------------------------------------------------------------------
def _device_collapse_backward(provider, device, mean, cov, lw, grads, **need):
    out = provider.switching_collapse_backward(*[_dev(x, device) for x in (mean, cov, lw) + tuple(grads)], **need)
    return out      # (grad_means, grad_covs, grad_log_weights)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,G,N,D", collapsed.COLLAPSE_SHAPES)
def test_the_collapse_backward_equals_the_contract(hip_device, B, G, N, D, shared):
    provider = _provider()
    mean, cov, lw = collapsed.example_collapse(B, G, N, D)
    if shared:
        mean, cov = np.ascontiguousarray(mean[:, 0]), np.ascontiguousarray(cov[:, 0])
    grads = backward.example_collapse_backward(B, G, N, D)
    want_lw, want_mean, want_cov = backward.switching_collapse_backward(mean, cov, lw, *grads)
    got = _device_collapse_backward(provider, hip_device, mean, cov, lw, grads)
    again = _device_collapse_backward(provider, hip_device, mean, cov, lw, grads)
    for name, value, repeat, reference in zip(("mean", "cov", "log_weight"), got, again, (want_mean, want_cov, want_lw)):
        assert tuple(value.shape) == reference.shape and value.dtype == torch.float64, name
        error, silent = slot_error(collapse_rows(value.cpu().numpy()), collapse_rows(reference))
        print(name, "largest error", error)
        assert silent and error <= LIMIT, name
        assert torch.equal(value, repeat), name
    for index, need in enumerate(("need_means", "need_covs", "need_log_weights")):
        only = dict(need_means=False, need_covs=False, need_log_weights=False)
        only[need] = True
        alone = _device_collapse_backward(provider, hip_device, mean, cov, lw, grads, **only)
        assert [part is None for part in alone] == [i != index for i in range(3)]
        assert torch.equal(alone[index], got[index]), need


@pytest.mark.parametrize("shared", [False, True])
def test_the_collapse_backwards_conventions_on_the_device(hip_device, shared):
    provider = _provider()
    mean, cov, lw = collapsed.example_collapse(2, 3, 4, 2)
    grads = backward.example_collapse_backward(2, 3, 4, 2)
    lw[0, 0, 1] = -np.inf
    lw[0, 1, :] = -np.inf                             # an empty group
    lw[1, 2, 0] = np.nan                              # a NaN weight
    if shared:
        mean, cov = np.ascontiguousarray(mean[:, 0]), np.ascontiguousarray(cov[:, 0])
        lw[0, :, 1] = -np.inf                         # dead under every group of row 0: not read by any
        mean[0, 1], cov[0, 1] = np.nan, np.nan
    else:
        mean[0, 0, 1], cov[0, 0, 1] = np.nan, np.nan  # a dead component is not read
    g_mean, g_cov, g_lw = (part.cpu().numpy() for part in _device_collapse_backward(provider, hip_device, mean, cov, lw, grads))
    want_lw, want_mean, want_cov = backward.switching_collapse_backward(mean, cov, lw, *grads)
    for value, reference in ((g_lw, want_lw), (g_mean, want_mean), (g_cov, want_cov)):
        assert np.array_equal(np.isnan(value), np.isnan(reference))
        assert np.array_equal(value == 0, reference == 0)
        # per slot against its own max|want|, a slot of scale 0 exactly zero; the NaN slots (equal above) set aside
        error, silent = slot_error(collapse_rows(np.nan_to_num(value)), collapse_rows(np.nan_to_num(reference)))
        assert silent and error <= LIMIT
    assert g_lw[0, 0, 1] == 0.0 and (g_lw[0, 1] == 0.0).all() and np.isnan(g_lw[1, 2]).all() and np.isfinite(g_lw[0]).all()
    if shared:
        assert (g_mean[0, 1] == 0.0).all() and (g_cov[0, 1] == 0.0).all() and np.isnan(g_mean[1]).all()
    else:
        assert (g_mean[0, 0, 1] == 0.0).all() and (g_mean[0, 1] == 0.0).all() and np.isnan(g_mean[1, 2]).all()
        assert np.isfinite(g_mean[1, :2]).all()


# ---- whole passes ---------------------------------------------------------------------------------------------------------------------------
def _wide_model():
    return contract.example_model(2, 8, 8, seed=4)


MODELS = {"2-2-1": lambda: contract.example_model(2, 2, 1), "3-3-2": lambda: contract.example_model(3, 3, 2),
          "4-2-2": lambda: contract.example_model(4, 2, 2), "2-8-8": _wide_model}
_REFERENCES = {}


def _reference(key, order, masked):
    """(observations, masks, value, gradients) of the CPU restatement, computed once per case and left unchanged."""
    case = (key, order, masked)
    if case not in _REFERENCES:
        T, B = 4, 3
        ops = MODELS[key]()
        observations = observations_of(ops, T, B)
        masks = None
        if masked:
            host = missing.example_masks(T, B, ops["C"].shape[-2], seed=1)
            masks = [None if t == 1 else torch.from_numpy(host[t]) for t in range(T)]
        leaves = leaves_of(ops)
        value = backward.collapsed_log_likelihood_restated(observations, leaves, order=order, observed=masks)
        weights = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
        grads = torch.autograd.grad((value * weights).sum(), list(leaves.values()))
        _REFERENCES[case] = (ops, observations, masks, value.detach(), dict(zip(PARAMETERS, grads)))
    return _REFERENCES[case]


# both orders, each plain and under a mask, in float64; float32 observations once per model (order 2, no mask)
PASSES = [(key, order, masked, torch.float64) for key in sorted(MODELS) for order in (2, 1) for masked in (False, True)] + \
    [(key, 2, False, torch.float32) for key in sorted(MODELS)]


@pytest.mark.parametrize("key,order,masked,y_dtype", PASSES)
def test_a_whole_pass_and_its_ten_gradients(hip_device, key, order, masked, y_dtype):
    from aesmc_amd import rao_blackwell
    ops, observations, masks, want, want_grads = _reference(key, order, masked)
    ys = [y.to(y_dtype) for y in observations]
    if y_dtype == torch.float32:      # the reference of the ROUNDED observations
        leaves = leaves_of(ops)
        want = backward.collapsed_log_likelihood_restated(ys, leaves, order=order)
        weights = torch.linspace(0.5, 1.5, want.numel(), dtype=torch.float64)
        want_grads = dict(zip(PARAMETERS, torch.autograd.grad((want * weights).sum(), list(leaves.values()))))
        want = want.detach()
    if masks is not None:
        ys = [y if m is None else torch.where(m, y, torch.full_like(y, float("nan"))) for y, m in zip(ys, masks)]
    ys = [y.to(hip_device) for y in ys]
    observed = None if masks is None else [None if m is None else m.to(hip_device) for m in masks]
    leaves = {name: value.detach().to(hip_device).requires_grad_(True) for name, value in leaves_of(ops).items()}
    value = rao_blackwell.collapsed_switching_log_likelihood(ys, leaves, order=order, observed=observed)
    assert value.shape == want.shape and value.dtype == torch.float64 and value.requires_grad
    model = rao_blackwell.SwitchingLinearGaussian(*[leaves[name].detach() for name in PARAMETERS])
    filtered = rao_blackwell.collapsed_switching_filter(ys, model, order=order, observed=observed)
    assert torch.equal(value.detach(), filtered["log_marginal_likelihood"])
    assert float((value.detach().cpu() - want).abs().max()) <= LIMIT * (1 + float(want.abs().max()))
    weights = torch.linspace(0.5, 1.5, value.numel(), dtype=torch.float64, device=hip_device)
    grads = torch.autograd.grad((value * weights).sum(), list(leaves.values()))
    assert_gradients({name: grad.cpu() for name, grad in zip(PARAMETERS, grads)}, want_grads)


def test_structural_zeros_on_the_device(hip_device):
    from aesmc_amd import rao_blackwell
    ops = contract.example_model(2, 2, 1, seed=3)
    ops = contract.operands(np.array([1.0, 0.0]), np.array([[1.0, 0.0], [0.4, 0.6]]), *[ops[name] for name in PARAMETERS[2:]])
    ops = dict(ops, C=ops["C"].copy(), r=ops["r"].copy())
    ops["C"][1], ops["r"][1] = 0.0, 0.0      # singular under regime 1, which step 0 excludes (pi0[1] = 0)
    observations = [y.to(hip_device) for y in observations_of(ops, 1, 2)]
    leaves = {name: value.detach().to(hip_device).requires_grad_(True) for name, value in leaves_of(ops).items()}
    value = rao_blackwell.collapsed_switching_log_likelihood(observations, leaves, order=2)
    grads = dict(zip(PARAMETERS, torch.autograd.grad(value.sum(), list(leaves.values()), allow_unused=True)))
    assert bool(torch.isfinite(value).all()) and grads["Pi"] is None      # (T == 1 does not read Pi)
    for name in PARAMETERS:
        assert name == "Pi" or bool(torch.isfinite(grads[name]).all()), name
    assert float(grads["pi0"][1]) == 0.0 and float(grads["C"][1].abs().max()) == 0.0 and float(grads["r"][1].abs().max()) == 0.0
    # and with exact zeros in Pi over several steps (regime 1 can be entered from regime 1 only, which pi0 excludes)
    ops = contract.example_model(2, 2, 1, seed=3)
    ops = contract.operands(np.array([1.0, 0.0]), np.array([[1.0, 0.0], [0.4, 0.6]]), *[ops[name] for name in PARAMETERS[2:]])
    series = observations_of(ops, 3, 2)
    theirs = leaves_of(ops)
    want = backward.collapsed_log_likelihood_restated(series, theirs, order=2)
    want_grads = dict(zip(PARAMETERS, torch.autograd.grad(want.sum(), list(theirs.values()))))
    leaves = {name: value.detach().to(hip_device).requires_grad_(True) for name, value in leaves_of(ops).items()}
    value = rao_blackwell.collapsed_switching_log_likelihood([y.to(hip_device) for y in series], leaves, order=2)
    grads = {name: grad.cpu() for name, grad in zip(PARAMETERS, torch.autograd.grad(value.sum(), list(leaves.values())))}
    assert float(grads["Pi"][0, 1]) == 0.0 and float(grads["pi0"][1]) == 0.0
    assert_gradients(grads, want_grads)


def test_one_optimiser_step_changes_every_parameter_and_lowers_the_loss(hip_device):
    from aesmc_amd import rao_blackwell
    truth = contract.example_model(2, 2, 2, seed=7)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(truth[name].copy()) for name in PARAMETERS])
    observations = [y.to(hip_device) for y in model.simulate(6, 16, seed=1)]
    start = contract.example_model(2, 2, 2, seed=8)
    raw = {name: torch.from_numpy(start[name].copy()).to(hip_device) for name in PARAMETERS}
    free = {name: (torch.log(raw[name]) if name in ("pi0", "Pi", "s0", "q", "r") else raw[name]).clone().requires_grad_(True)
            for name in PARAMETERS}

    def parameters():
        out = {name: free[name] for name in ("m0", "A", "b", "C", "d")}
        out.update(pi0=torch.softmax(free["pi0"], dim=-1), Pi=torch.softmax(free["Pi"], dim=-1))
        out.update({name: torch.exp(free[name]) for name in ("s0", "q", "r")})
        return out

    before = {name: value.detach().clone() for name, value in free.items()}
    optimiser = torch.optim.SGD(list(free.values()), lr=1e-3)
    loss = rao_blackwell.collapsed_switching_loss(observations, parameters())
    optimiser.zero_grad()
    loss.backward()
    for name, value in free.items():
        assert value.grad is not None and bool(torch.isfinite(value.grad).all()) and float(value.grad.abs().max()) > 0, name
    optimiser.step()
    for name, value in free.items():
        assert not torch.equal(value.detach(), before[name]), name
    with torch.no_grad():
        after = rao_blackwell.collapsed_switching_loss(observations, parameters())
    print("loss", float(loss), "->", float(after))
    assert float(after) < float(loss)
