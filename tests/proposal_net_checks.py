"""What the tests of the proposal net (kernels K13 / K13b: out = b2 + W2 tanh(c1[b] + W1 x)) share: operands, the float64
reference, the eager float32 stand-in that sets a limit, and metrics under which a wrong gradient of ONE particle, a
hidden unit left out of it or a tanh that is 1e-5 off cannot hide.

The metric these replace took max|got - want| over a whole tensor relative to its largest entry, with 6e-5 allowed in
float32.  Here, with Bk = |G W2| [B,K,H] the size of what reaches each hidden unit of each particle:

  * grad_x, per particle: err[b,k] = max_i |got - want| / A[b,k], A[b,k] = max_i sum_h |W1[h,i]| (1 - h^2) Bk[b,k,h] —
    the absolute sum of the particle's own terms; where A is 0 the row has to be exactly zero.  On saturated inputs
    (offsets shifted by 4 .. 1e4) A', the same without the factor (1 - h^2): float32 holds h, not 1 - h^2, to relative
    accuracy there (h = 0.9993 is 6e-8 off, 1 - h^2 = 1.3e-3 then 1e-4 of itself), and eager autograd does no better.
    The sums over particles that carry the factor (grad_c1, grad_W1) are measured likewise on such inputs: against the
    largest entry of the absolute sum of their terms without it.
  * grad_c1 [B,H], per batch row: max_h |got - want| / max_h |want[b]|; a row nothing reaches is exactly zero.
  * grad_W1, grad_W2, grad_b2 and a shared [H] offset's gradient: gradient_checks.reduced_error, no floor.
  * forward, per element: |got - want| / (|b2[o]| + sum_h |W2[o,h]| |h_h|).

Limits as in tests/gradient_checks.py: float32 max(8 e_ref, 16 eps32) with e_ref the stand-in's error under the same
metric on the same inputs, output by output; float64 1e-10.  Inputs whose 8 e_ref exceeds 1e-4 are changed, never the
factor.
"""
import math

import numpy as np
import torch

from tests import gradient_checks as gc

REGIMES = ("flat", "probes", "probes_last_row")
NAMES = ("x", "W1", "c1", "W2", "b2")
SHIFTS = (4.0, 9.0, 20.0, 1.0e4)


# ---- operands ---------------------------------------------------------------------------------------------------------
def operands(B, K, din, H, dout, dtype, device, seed, shared_offset=False):
    """{x [B,K,din], W1 [H,din], c1 [B,H] (or [H]), W2 [dout,H], b2 [dout]} of `dtype` on `device`, drawn in float64 on
    the host and rounded."""
    r = np.random.RandomState(seed).randn
    host = {"x": r(B, K, din), "W1": r(H, din) / np.sqrt(din), "c1": r(B, H), "W2": r(dout, H) / np.sqrt(H), "b2": r(dout)}
    if shared_offset:
        host["c1"] = host["c1"][0]
    return {name: torch.from_numpy(np.ascontiguousarray(value)).to(dtype).to(device) for name, value in host.items()}


def upstream(regime, B, K, dout, dtype, device, seed):
    """G [B,K,dout]: randn (`flat`), or randn at gradient_checks.probe_positions(K) of every batch row (`probes`) or of
    the last one only (`probes_last_row`) and exactly 0 elsewhere."""
    assert regime in REGIMES, regime
    full = np.random.RandomState(seed).randn(B, K, dout)
    if regime == "flat":
        host = full
    else:
        host = np.zeros_like(full)
        rows = range(B) if regime == "probes" else [B - 1]
        for b in rows:
            host[b, gc.probe_positions(K)] = full[b, gc.probe_positions(K)]
    return torch.from_numpy(host).to(dtype).to(device)


def saturate(o, fully_saturated_row=None, at_least=20.0):
    """The operands with c1 [B,H] shifted by +4, -4, +9, -9, +20, -20, +1e4, -1e4, ... along the hidden units (the signs
    the other way round in every other batch row); in `fully_saturated_row` every shift is `at_least` or more."""
    c1 = o["c1"].double().cpu()
    B, H = c1.shape
    size = torch.tensor([SHIFTS[(h // 2) % len(SHIFTS)] for h in range(H)], dtype=torch.float64)
    sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(H)], dtype=torch.float64)
    shift = torch.stack([(sign if b % 2 == 0 else -sign) * size for b in range(B)])
    if fully_saturated_row is not None:
        row = shift[fully_saturated_row]
        shift[fully_saturated_row] = torch.sign(row) * row.abs().clamp(min=at_least)
    out = dict(o)
    out["c1"] = (c1 + shift).to(o["c1"].dtype).to(o["c1"].device)
    return out


# ---- the expression, its float64 reference and its eager float32 stand-in -------------------------------------------------
def expression(x, W1, c1, W2, b2=None, tanh=torch.tanh):
    z = torch.matmul(x, W1.t()) + (c1.unsqueeze(1) if c1.dim() == 2 else c1)
    out = torch.matmul(tanh(z), W2.t())
    return out if b2 is None else out + b2


def autograd(o, G, dtype, with_b2=False, tanh=torch.tanh):
    """{name: gradient of sum(G * expression)} in `dtype` on the operands' device, and the forward values under "out"."""
    names = [name for name in NAMES if name != "b2" or with_b2]
    leaves = {name: o[name].detach().to(dtype).clone().requires_grad_(True) for name in names}
    out = expression(leaves["x"], leaves["W1"], leaves["c1"], leaves["W2"], leaves.get("b2"), tanh=tanh)
    grads = torch.autograd.grad(out, [leaves[name] for name in names], G.detach().to(dtype))
    result = dict(zip(names, grads))
    result["out"] = out.detach()
    return result


def hidden(o):
    """(z, h = tanh z) [B,K,H] in float64 from the rounded operands."""
    x, W1, c1 = o["x"].double(), o["W1"].double(), o["c1"].double()
    z = torch.matmul(x, W1.t()) + (c1.unsqueeze(1) if c1.dim() == 2 else c1)
    return z, torch.tanh(z)


def reference(o, G, with_b2=False):
    """float64 autograd of the expression on the rounded operands: the gradients, "out", and "z", "h"."""
    want = autograd(o, G, torch.float64, with_b2=with_b2)
    want["z"], want["h"] = hidden(o)
    return want


def stand_in(o, G, with_b2=False):
    """Eager float32 autograd of the same expression on the same device: it measures e_ref and is never the kernel."""
    return autograd(o, G, torch.float32, with_b2=with_b2)


# ---- scales -----------------------------------------------------------------------------------------------------------------
def reach(o, G):
    """Bk = |G W2| [B,K,H] in float64."""
    return torch.matmul(G.double(), o["W2"].double()).abs()


def scales(o, G, want, saturated=False):
    """{"x": A [B,K] (A' if `saturated`)}; if `saturated` also "c1" [B] and "W1" (a number): the largest entry of the
    absolute sum of the terms without the factor (1 - h^2)."""
    Bk = reach(o, G)
    W1 = o["W1"].double().abs()
    if not saturated:
        return {"x": torch.matmul(Bk * (1.0 - want["h"] ** 2), W1).amax(dim=-1)}
    absolute_w1 = torch.einsum("bkh,bki->hi", Bk, o["x"].double().abs())
    return {"x": torch.matmul(Bk, W1).amax(dim=-1), "c1": Bk.sum(dim=1).amax(dim=-1), "W1": float(absolute_w1.max())}


# ---- metrics ----------------------------------------------------------------------------------------------------------------
def absolute_error(got, want, size):
    """max|got - want| / size for a sum measured against the absolute sum of its terms."""
    got, want = got.double().reshape(want.shape), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    diff = float((got - want).abs().max())
    if size == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / size


def rows_shape(got, want):
    """grad_c1 as [B,H] whatever the offset's own shape."""
    return got.reshape(want.shape) if got.numel() == want.numel() else got


def measure(got, want, sc):
    """{name: error} for the gradients present in `got` (a dict; None entries are passed over), and "silent": whether
    every particle / batch row that nothing reaches is exactly zero."""
    out, silent = {}, True
    for name in NAMES:
        value = got.get(name)
        if value is None:
            continue
        reference_ = want[name]
        if name == "x":
            assert value.shape == reference_.shape, name
            out[name], quiet = gc.particle_error(value, reference_, sc["x"])
            silent = silent and quiet
        elif name == "c1" and reference_.dim() == 2 and "c1" in sc:
            assert value.shape == reference_.shape, name
            counted = sc["c1"] > 0
            out[name] = max([absolute_error(value[b], reference_[b], float(sc["c1"][b])) for b in range(len(counted))
                             if bool(counted[b])] or [0.0])
            silent = silent and (bool((value[~counted] == 0).all()) if bool((~counted).any()) else True)
        elif name == "c1" and reference_.dim() == 2:
            assert value.shape == reference_.shape, name
            out[name], quiet = gc.particle_error(value, reference_, reference_.abs().amax(dim=-1))
            silent = silent and quiet
        elif name == "W1" and "W1" in sc:
            out[name] = absolute_error(value, reference_, sc["W1"])
        else:
            assert value.numel() == reference_.numel(), name
            out[name] = gc.reduced_error(value, reference_)
    out["silent"] = silent
    return out


def limits(reference_errors, dtype):
    """The limit of every output from the stand-in's error in the same output."""
    if dtype == torch.float64:
        return {name: gc.FLOAT64_TOLERANCE for name in NAMES}
    return {name: gc.tolerance(err) for name, err in reference_errors.items() if name != "silent"}


def check(got, want, sc, stand_in_grads=None, what=""):
    """Assert the gradients in `got` against `want`.  `stand_in_grads`: the eager float32 gradients that set the limits;
    None: the float64 limit.  Returns (errors, the stand-in's errors or None, limits)."""
    mine = measure(got, want, sc)
    if stand_in_grads is None:
        reference_errors, allowed = None, limits(None, torch.float64)
    else:
        reference_errors = measure({name: stand_in_grads.get(name) for name in got if got[name] is not None}, want, sc)
        allowed = limits(reference_errors, torch.float32)
    assert mine["silent"], "{}: a particle or batch row that nothing reaches has a nonzero gradient".format(what)
    for name, err in mine.items():
        if name != "silent":
            assert err <= allowed[name], "{}: grad_{} error {:.3e} > {:.3e} ({})".format(what, name, err, allowed[name], mine)
    return mine, reference_errors, allowed


def forward_error(got, want, o, with_b2=True):
    """The largest |got - want| / (|b2[o]| + sum_h |W2[o,h]| |h_h|) over the elements."""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    size = torch.matmul(want["h"].abs(), o["W2"].double().abs().t())
    if with_b2:
        size = size + o["b2"].double().abs()
    return float(((got.double() - want["out"]).abs() / size).max())


def check_forward(got, want, o, stand_in_out=None, with_b2=True, what=""):
    """Returns (error, e_ref or None, limit)."""
    err = forward_error(got, want, o, with_b2)
    e_ref = None if stand_in_out is None else forward_error(stand_in_out, want, o, with_b2)
    limit = gc.FLOAT64_TOLERANCE if stand_in_out is None else gc.tolerance(e_ref)
    assert math.isfinite(err) and err <= limit, "{}: forward error {:.3e} > {:.3e}".format(what, err, limit)
    return err, e_ref, limit


def earlier_metric(got, want):
    """What test_particle_mlp_backward_equals_float64_autograd reads: the largest, over the outputs, of max|got - want| over
    the tensor's largest entry (its float32 limit: 6e-5)."""
    worst = 0.0
    for name in NAMES:
        if got.get(name) is not None:
            reference_ = want[name].double()
            worst = max(worst, float((got[name].double().reshape(reference_.shape) - reference_).abs().max()) /
                        max(float(reference_.abs().max()), 1e-30))
    return worst
