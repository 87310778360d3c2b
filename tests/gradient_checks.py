"""What the backward tests of the linear-Gaussian step share: references, weights under which every particle counts, and
two metrics that a wrong gradient of ONE particle cannot hide under.

A step's log-weights on `randn` operands leave an effective sample size of about two per batch row, and a max norm
floored at 1 then sees the two particles that hold the weight and nobody else.  The backward entry points take the
log-weights `lw` and their row log-sum-exp `lse` as DATA (they read them only to form g = grad_lse * exp(lw - lse)), so
the tests hand in weights of their own:

  * flat:   lw = randn(B, K) — an effective sample size near K / 2.7, asserted >= K / 4 per row;
  * probes: lw = -1e4 except at a few named particles per row (0), so that exp underflows to exactly 0 everywhere else
            and the reduced gradients are the sum over just the probes.

Per-particle outputs (the gradient of x_{t-1}'s rows; of x_t's for the log-weight kernel) are measured particle by
particle against each particle's own size: with U the float64 gradient for g = 1 and nothing arriving at x_t, V the one
for g = 0 and the given `grad_x`,

    scale[b,k] = |g[b,k]| * max|U[b,k,:]| + max|V[b,k,:]|,      err[b,k] = max|got - want|[b,k,:] / scale[b,k],

and where scale is 0 the output row has to be exactly zero.  Reduced outputs (weights, offsets, scales, y) are measured
as max|got - want| / max|want|, with no floor of 1.  The limit is not a constant: every case measures e_ref, the error
of eager float32 PyTorch autograd of the same expression on the same inputs under the same metric, and allows
max(8 e_ref, 16 eps32) (a different, fixed summation order and the hardware's exp inside g; a dropped, doubled or
misplaced particle is an error of order 1).  A case whose 8 e_ref exceeds 1e-4 is ill-conditioned: its inputs change,
never the factor.
"""
import math

import numpy as np
import torch

SLOTS = ("x_prev", "x", "y", "A", "off_p", "C", "off_g", "Q", "off_q", "s_p", "s_g", "s_q")
PARAMETERS = ("y", "A", "off_p", "C", "off_g", "Q", "off_q", "s_p", "s_g", "s_q")
EPS32 = float(np.finfo(np.float32).eps)
FLOAT64_TOLERANCE = 1e-10
CONDITION_LIMIT = 1e-4
PROBES = (0, 63, 64, 255, 256)      # and K - 1: both sides of a wavefront's and of a 256-particle tile's edge


# ---- operands ---------------------------------------------------------------------------------------------------------
def step_operands(B, K, dx, dy, dtype, device, seed, matched=False, spread=0.1, emission=0.3):
    """The operands of one step as tensors of `dtype` on `device` (drawn in float64 on the host): x_prev, eps, y, the
    three maps, their offsets (transition's shared, emission's shared, proposal's per batch row) and scales.
    `matched`: transition equal to proposal (A = Q, equal offsets) and a weak emission (C = 0.02 randn, s_g = 1) — the
    model whose OWN log-weights are nearly flat.  Its scales are close, not equal (s_p = 0.75 against s_q = 0.7): with
    equal ones x_t is an exact draw from the transition, the gradient of s_p — the sum of g (|r|^2 / s^3 - d / s) — has
    terms of mean zero, and float32 autograd itself is then 1e-5 off it; the log-weights stay flat (ESS near K / 2)."""
    rng = np.random.RandomState(seed)
    r = rng.randn
    host = {"x_prev": r(B, K, dx), "eps": r(B, K, dx), "y": r(B, dy),
            "A": 0.9 * np.eye(dx) + spread * r(dx, dx), "off_p": r(dx),
            "C": emission * r(dy, dx), "off_g": r(dy),
            "Q": 0.45 * np.eye(dx) + spread * r(dx, dx), "off_q": r(B, dx),
            "s_p": np.asarray(1.0), "s_g": np.asarray(0.5), "s_q": np.asarray(0.7)}
    if matched:
        host.update(A=host["Q"].copy(), off_p=host["off_q"].copy(), s_p=np.asarray(0.75),
                    C=0.02 * r(dy, dx), s_g=np.asarray(1.0))
    return {name: torch.from_numpy(np.ascontiguousarray(value)).to(dtype).to(device) for name, value in host.items()}


def draw(operands, ancestors=None, noise_scale=None):
    """x_t = loc_q(x_{t-1}[ancestors]) + s_q eps, formed in float64 and rounded to the operands' dtype; `noise_scale` in
    place of s_q for a latent that is NOT the proposal's draw.  (Rounded from float64, x_t is data to everybody alike:
    formed by float32 matmul it would be bit for bit what eager float32 autograd subtracts again to recover eps, and
    the stand-in that sets the limit would be spared a rounding that every other implementation meets.)"""
    x_prev = operands["x_prev"].double()
    moved = x_prev if ancestors is None else gather_rows(x_prev, ancestors)
    scale = operands["s_q"].double() if noise_scale is None else noise_scale
    x = moved @ operands["Q"].double().t() + _rows(operands["off_q"].double()) + scale * operands["eps"].double()
    return x.to(operands["x_prev"].dtype)


def arriving_gradient(operands, seed, index=None):
    """A gradient of order 1 arriving at x_t from later steps: randn + eps / 2, of the rows `index` names where given
    (one row per child).  The part along eps keeps the proposal scale's gradient — the sum over ALL particles of
    grad_x . eps — well-conditioned: pure noise sums to sqrt(B K d) of its terms' size, or by chance to far less, and
    then float32 autograd itself is 1e-5 off."""
    eps = operands["eps"]
    gen = torch.Generator().manual_seed(seed)
    noise = torch.randn(eps.shape, generator=gen, dtype=torch.float64).to(eps.dtype).to(eps.device)
    return noise + 0.5 * (eps if index is None else gather_rows(eps, index))


def gather_rows(value, index):
    return torch.gather(value, 1, index.unsqueeze(-1).expand(-1, -1, value.size(2)))


def sorted_indices(B, K, seed, device):
    """int64 [B, K], every row sorted, with repeats and gaps (K draws with replacement); the LAST row (where B > 1)
    names one particle only: every child has the same parent."""
    rng = np.random.RandomState(seed)
    index = np.sort(rng.randint(0, K, size=(B, K)), axis=1)
    if B > 1:
        index[-1] = K // 3
    return torch.from_numpy(index.astype(np.int64)).to(device)


def child_ranges(next_ancestors):
    """child_end[b,k] = #{k' : next_ancestors[b,k'] <= k} (int32): particle k's children are the rows
    child_end[b,k-1] .. child_end[b,k] - 1 of the next step."""
    host = next_ancestors.cpu().numpy()
    K = host.shape[1]
    ends = np.stack([np.searchsorted(row, np.arange(K), side="right") for row in host])
    return torch.from_numpy(ends.astype(np.int32)).to(next_ancestors.device)


def sum_children(child_grad, next_ancestors, dtype=torch.float64):
    """torch.gather's backward: every child's row added to its parent's, in `dtype`."""
    B, K, d = child_grad.shape
    flat = (next_ancestors + K * torch.arange(B, device=child_grad.device).unsqueeze(1)).reshape(-1)
    out = torch.zeros(B * K, d, dtype=dtype, device=child_grad.device)
    return out.index_add_(0, flat, child_grad.to(dtype).reshape(B * K, d)).view(B, K, d)


# ---- weights under which every particle counts -----------------------------------------------------------------------------
def effective_sample_size(lw):
    w = torch.softmax(lw.double(), dim=1)
    return 1.0 / (w * w).sum(dim=1)


def assert_flat(lw):
    K = lw.size(1)
    ess = effective_sample_size(lw)
    assert float(ess.min()) >= K / 4.0, "weights too peaked for this check: ESS {} of {} particles".format(ess.tolist(), K)


def finish_weights(lw64, dtype, device):
    """(lw, lse) of `dtype`: lse the float64 log-sum-exp of the ROUNDED lw, rounded."""
    lw = lw64.to(dtype)
    lse = torch.logsumexp(lw.double(), dim=1).to(dtype)
    return lw.to(device), lse.to(device)


def flat_weights(B, K, dtype, device, seed):
    """lw = randn(B, K): an effective sample size near K / e.  One draw in a few has a row with a particle four standard
    deviations out that takes a tenth of the weight: such a draw is passed over for the next (at most sixteen)."""
    for attempt in range(16):
        gen = torch.Generator().manual_seed(seed + 7919 * attempt)
        lw64 = torch.randn(B, K, generator=gen, dtype=torch.float64)
        if float(effective_sample_size(lw64.to(dtype)).min()) >= K / 4.0:
            break
    lw, lse = finish_weights(lw64, dtype, device)
    assert_flat(lw)
    return lw, lse


def probe_positions(K):
    return sorted({k for k in PROBES + (K - 1,) if 0 <= k < K})


def probe_weights(B, K, dtype, device, rows=None):
    """(lw, lse, has_probes [B] bool): lw = 0 at `probe_positions(K)` of the batch rows in `rows` (default: all), -1e4
    elsewhere — exp(lw - lse) is exactly 0 off the probes.  A row without probes has no particle that counts: the
    caller hands it grad_lse = 0."""
    rows = list(range(B)) if rows is None else list(rows)
    lw64 = torch.full((B, K), -1.0e4, dtype=torch.float64)
    for b in rows:
        lw64[b, probe_positions(K)] = 0.0
    has = torch.zeros(B, dtype=torch.bool)
    has[rows] = True
    lw, lse = finish_weights(lw64, dtype, device)
    return lw, lse, has.to(device)


def softmax_term(lw, lse, grad_lse):
    """g = grad_lse * exp(lw - lse) in float64 from the very values handed to the kernel."""
    return grad_lse.double().unsqueeze(1) * torch.exp(lw.double() - lse.double().unsqueeze(1))


FEW_TERMS = 64
CANCELLATION_LIMIT = 8.0


def well_conditioned(stand_in, want, scales, g=None, cancellation=None):
    """Are these inputs fit to judge a float32 kernel on?  Two conditions, neither of which looks at the kernel:
      * eager float32 autograd itself is within CONDITION_LIMIT / 8 of `want` under both metrics (a particle whose own
        terms cancel to a fiftieth of their size — one in a thousand does at rows of two values — fails this);
      * where at most FEW_TERMS particles count (the probes), no scale's gradient cancels to less than an eighth of its
        terms' absolute sum (`cancellation`, a function that measures it): the error of a float32 sum of a handful of
        terms is of the order of eps32 times that absolute sum, a couple of eps32 with the terms' own roundings, and
        the floor of the limit, 16 eps32, has to hold it whether or not eager autograd happened to round luckily.  (Six
        probes in one batch row summed to a hundredth of their sizes in one case, where the stand-in was 1e-6 off
        and the kernel 8e-6: 8e-8 of the terms.)
    Inputs that fail are drawn again, and a test asserts that the draw it goes on with passed; the factor 8 stays.
    (The second condition is more than the e_ref rule asks: without it the limit of a six-term sum depends on whether
    eager autograd's own roundings happened to cancel.)"""
    reference = measure(stand_in, want, scales)
    if 8.0 * max(reference["particle"], reference["reduced"]) > CONDITION_LIMIT:
        return False
    if g is not None and cancellation is not None and int((g != 0).sum()) <= FEW_TERMS:
        return cancellation() <= CANCELLATION_LIMIT
    return True


# ---- references -------------------------------------------------------------------------------------------------------------
def _rows(offset):
    if offset is None:
        return 0.0
    return offset.unsqueeze(1) if offset.dim() == 2 else offset


def log_weight(xp, x, y, A, off_p, C, off_g, Q, off_q, s_p, s_g, s_q):
    """log p(x_t | x_{t-1}) + log g(y | x_t) - log q(x_t | x_{t-1}) [B, K], as the reference states it."""
    normal = lambda loc, scale: torch.distributions.Normal(loc, scale, validate_args=False)
    return (normal(xp @ A.t() + _rows(off_p), s_p).log_prob(x).sum(-1) +
            normal(x @ C.t() + _rows(off_g), s_g).log_prob(y.unsqueeze(1)).sum(-1) -
            normal(xp @ Q.t() + _rows(off_q), s_q).log_prob(x).sum(-1))


def _leaves(operands, dtype, **replaced):
    leaves = {}
    for name in ("x_prev",) + PARAMETERS:
        value = replaced.get(name, operands.get(name))
        leaves[name] = None if value is None else value.detach().to(dtype).clone().requires_grad_(True)
    return leaves


def _grads(total, leaves, names):
    present = [name for name in names if leaves.get(name) is not None]
    grads = torch.autograd.grad(total, [leaves[name] for name in present], allow_unused=True)
    out = [None] * 12
    for name, grad in zip(present, grads):
        out[SLOTS.index(name)] = torch.zeros_like(leaves[name]) if grad is None else grad
    return out


def _step_objective(leaves, x, g, grad_x, dtype):
    loc_q = leaves["x_prev"] @ leaves["Q"].t() + _rows(leaves["off_q"])
    with torch.no_grad():
        eps = (x.to(dtype) - loc_q) / leaves["s_q"]
    x_t = loc_q + leaves["s_q"] * eps
    value = log_weight(leaves["x_prev"], x_t, *[leaves[name] for name in PARAMETERS])
    total = (value * g.to(dtype)).sum()
    if grad_x is not None:
        total = total + (x_t * grad_x.to(dtype)).sum()
    return total


def step_reference(operands, x, g, grad_x, ancestors=None, dtype=torch.float64):
    """Autograd (float64; `dtype` = float32 gives the eager float32 stand-in that sets the limit) of one step whose x_t
    is rebuilt as the proposal's draw loc_q(x_prev) + s_q eps, eps held fixed: the twelve slots for
    sum(g * log_weight) + sum(grad_x * x_t).  With `ancestors` slot 0 is the gradient of the RESAMPLED rows
    x_prev[b, ancestors[b,k]], as the kernel returns it."""
    moved = operands["x_prev"] if ancestors is None else gather_rows(operands["x_prev"], ancestors)
    leaves = _leaves(operands, dtype, x_prev=moved)
    return _grads(_step_objective(leaves, x, g, grad_x, dtype), leaves, ("x_prev",) + PARAMETERS)


def _log_weight_objective(leaves, g, dtype):
    value = log_weight(leaves["x_prev"], leaves["x"], *[leaves[name] for name in PARAMETERS])
    return (value * g.to(dtype)).sum()


def log_weight_reference(operands, x, g, dtype=torch.float64):
    """The same for the log-weight kernel alone: x a leaf (slot 1), nothing else arriving at it."""
    leaves = _leaves(operands, dtype)
    leaves["x"] = x.detach().to(dtype).clone().requires_grad_(True)
    return _grads(_log_weight_objective(leaves, g, dtype), leaves, ("x_prev", "x") + PARAMETERS)


def _cancellation(total, leaves):
    shares = torch.autograd.grad(total, [leaves[name] for name in ("s_p", "s_g", "s_q")], allow_unused=True)
    worst = 1.0
    for share in shares:
        if share is not None and float(share.abs().sum()) > 0.0:
            worst = max(worst, float(share.abs().sum()) / max(float(share.sum().abs()), 1e-300))
    return worst


def _per_particle_scales(leaves, operands, shape):
    for name in ("s_p", "s_g", "s_q"):
        leaves[name] = operands[name].detach().double().reshape(1, 1, 1).expand(*shape, 1).clone().requires_grad_(True)


def step_scale_cancellation(operands, x, g, grad_x, ancestors=None):
    """How far the particles' shares of a scale's gradient cancel: the largest, over s_p, s_g and s_q, of
    sum_k |c_k| / |sum_k c_k| (float64, one pass: every particle is given a scale of its own and c is the gradient)."""
    moved = operands["x_prev"] if ancestors is None else gather_rows(operands["x_prev"], ancestors)
    leaves = _leaves(operands, torch.float64, x_prev=moved)
    _per_particle_scales(leaves, operands, g.shape)
    return _cancellation(_step_objective(leaves, x, g, grad_x, torch.float64), leaves)


def log_weight_scale_cancellation(operands, x, g):
    leaves = _leaves(operands, torch.float64)
    leaves["x"] = x.detach().double()
    _per_particle_scales(leaves, operands, g.shape)
    return _cancellation(_log_weight_objective(leaves, g, torch.float64), leaves)


def step_particle_scale(operands, x, g, grad_x, ancestors=None):
    """scale[b,k] of the step's slot 0 (float64): |g| max|U| + max|V|."""
    one, zero = torch.ones_like(g, dtype=torch.float64), torch.zeros_like(g, dtype=torch.float64)
    U = step_reference(operands, x, one, None, ancestors)[0]
    scale = g.double().abs() * U.abs().amax(dim=-1)
    if grad_x is not None:
        scale = scale + step_reference(operands, x, zero, grad_x, ancestors)[0].abs().amax(dim=-1)
    return scale


def log_weight_particle_scales(operands, x, g):
    """{slot: scale[b,k]} for slots 0 and 1 of the log-weight kernel: |g| max|U| (nothing else arrives)."""
    unit = log_weight_reference(operands, x, torch.ones_like(g, dtype=torch.float64))
    return {slot: g.double().abs() * unit[slot].abs().amax(dim=-1) for slot in (0, 1)}


# ---- metrics ----------------------------------------------------------------------------------------------------------------
def particle_error(got, want, scale):
    """(the largest err[b,k] over the particles with scale > 0, whether every row with scale == 0 is exactly zero)."""
    diff = (got.double() - want.double()).abs().amax(dim=-1)
    counted = scale > 0
    worst = float((diff[counted] / scale[counted]).max()) if bool(counted.any()) else 0.0
    silent = bool((got[~counted] == 0).all()) if bool((~counted).any()) else True
    if not math.isfinite(worst) or not bool(torch.isfinite(got).all()):
        worst = float("inf")
    return worst, silent


def reduced_error(got, want):
    """max|got - want| / max|want|; a reference that is zero everywhere asks for an output that is exactly zero."""
    got, want = got.double().reshape(want.shape), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    size = float(want.abs().max())
    diff = float((got - want).abs().max())
    if size == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / size


def measure(got, want, scales):
    """Both metrics over the slots of `want`: {"particle": worst, "reduced": worst, "silent": bool, "slots": {name: err}}.
    `scales` maps a per-particle slot to its scale[b,k]; every other slot present in `want` is a reduced output."""
    out = {"particle": 0.0, "reduced": 0.0, "silent": True, "slots": {}}
    for slot, reference in enumerate(want):
        if reference is None:
            continue
        assert got[slot] is not None, "no gradient for " + SLOTS[slot]
        if slot in scales:
            assert got[slot].shape == reference.shape, SLOTS[slot]
            err, silent = particle_error(got[slot], reference, scales[slot])
            out["particle"] = max(out["particle"], err)
            out["silent"] = out["silent"] and silent
        else:
            assert got[slot].numel() == reference.numel(), SLOTS[slot]
            err = reduced_error(got[slot], reference)
            out["reduced"] = max(out["reduced"], err)
        out["slots"][SLOTS[slot]] = err
    return out


def tolerance(e_ref):
    """The limit for a float32 kernel whose eager float32 stand-in measured `e_ref` on the same inputs."""
    assert 8.0 * e_ref <= CONDITION_LIMIT, \
        "ill-conditioned inputs: eager float32 autograd is already {:.2e} off — change the inputs, not the factor".format(e_ref)
    return max(8.0 * e_ref, 16.0 * EPS32)


def check(got, want, scales, stand_in=None, what=""):
    """Assert `got` against `want` under both metrics.  `stand_in`: the eager float32 slots that set the limit; None: the
    float64 limit.  Returns the figures: (kernel's measure, stand-in's measure or None, (limit per-particle, reduced))."""
    mine = measure(got, want, scales)
    if stand_in is None:
        reference, limits = None, (FLOAT64_TOLERANCE, FLOAT64_TOLERANCE)
    else:
        reference = measure(stand_in, want, scales)
        limits = (tolerance(reference["particle"]), tolerance(reference["reduced"]))
    assert mine["silent"], "{}: a particle that nothing reaches has a nonzero gradient".format(what)
    assert mine["particle"] <= limits[0], "{}: per-particle error {:.3e} > {:.3e} ({})".format(
        what, mine["particle"], limits[0], mine["slots"])
    assert mine["reduced"] <= limits[1], "{}: reduced error {:.3e} > {:.3e} ({})".format(
        what, mine["reduced"], limits[1], mine["slots"])
    return mine, reference, limits
