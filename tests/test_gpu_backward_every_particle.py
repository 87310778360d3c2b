"""The backward kernels of the linear-Gaussian step against float64 autograd with EVERY particle counting.

The other backward tests hand a kernel the forward step's own log-weights on `randn` operands (an effective sample size
of about two per batch row, 1.0000 at rows of 128 values) and compare in a max norm floored at 1: the gradient of all
but the two particles that hold the weight could be zero and they would pass.  Here the kernels get log-weights as data
(tests/gradient_checks.py: flat, and probes at particles 0, 63, 64, 255, 256, K - 1 with exp(lw - lse) exactly 0
elsewhere — in every row, then in the last batch row only) and are measured particle by particle against each
particle's own gradient size, the reduced outputs (weights, offsets, scales, y) relative to their own largest entry,
without a floor.  Each float32 case takes its limit from e_ref, the error of eager float32 PyTorch autograd of the same
expression on the device on the same inputs: max(8 e_ref, 16 eps32); float64: 1e-10.  One case per family runs on the
launch's OWN log-weights, on a model matched so that they are flat (transition = proposal, weak emission).

Families, and the form each case asserts it ran:
  * K14 rows form (float32 rows of 2 .. 14 values, K a multiple of 256) — form 2, incl. three workgroups over sixteen
    tiles, so that the loads issued one tile ahead and the column sums at a tile's end carry over;
  * K14 general form — form 1 forced, the same shapes plus ragged and non-square ones, float32 and float64, one
    particle per lane; two per lane at a size that takes it (10 latent, 11 observed values, 2^20 particles); a row of one
    particle is declined and goes the unfused route (counted);
  * two chained steps — the later defers its parameter sums, the earlier carries them: both steps' sum;
  * K12 on (lw, lse, grad_lse), both latents' gradients per particle — one and (2^20 particles) two per lane;
  * the wide backward, the recomputing adjoint: at rows of 128 values in whole tiles of 256 particles through its
    hand-written passes (aesmc_wide_adjoint_scale / _merge, each counted once per case, `grad_x` handed to the second
    as its `add` operand and absent); at the other widths (24 .. 256) and at K = 320, where the element-wise parts are
    PyTorch's operations, those passes counted NOT to run.
Particles per lane are asserted from the launcher's own record (aesmc_test_last_affine_backward_particles_per_lane).
Through the ancestors (sorted, repeats, gaps, a row whose children all have one parent), with the next step's per-child
gradient and its children ranges (through identity ancestors), with both, with and without a gradient arriving at x_t.

Inputs on which float32 cannot be judged are drawn again (tests/gradient_checks.py `well_conditioned`: eager float32
autograd itself more than 1.25e-5 off, or — probes — a scale's gradient whose few terms cancel to less than an eighth of
their absolute sum), and every case asserts that the draw it uses is well-conditioned: 907 of 955 cases use the first
draw, none needs more than five; no case needed 8 e_ref > 1e-4.

Measured on an MI355X, per-particle metric / reduced metric, the worst over the family's cases (every case's limit is
max(8 e_ref, 16 eps32 = 1.9e-6) from its own e_ref; the last column is the case that came closest to its limit):

  family (float32)           cases   e_ref              largest limit      kernel error       error / limit
  K14 rows form               208    2.3e-6 / 1.8e-6    1.8e-5 / 1.4e-5    1.5e-6 / 8.2e-7    0.24 / 0.43
  K14 general form            324    2.1e-6 / 5.1e-6    1.7e-5 / 4.0e-5    4.9e-6 / 2.3e-6    0.30 / 0.47
  K14 on its own weights        3    3.3e-7 / 5.8e-7    2.7e-6 / 4.7e-6    4.2e-7 / 1.1e-6    0.17 / 0.23
  K14 chained                   4    2.9e-7 / 1.9e-7    2.3e-6 / 1.9e-6    3.6e-7 / 2.0e-7    0.16 / 0.10
  K12                          15    3.0e-6 / 7.3e-6    2.4e-5 / 5.8e-5    2.5e-6 / 8.0e-6    0.17 / 0.26
  wide, fused passes           24    1.3e-6 / 1.9e-6    1.1e-5 / 1.5e-5    1.3e-6 / 2.0e-6    0.18 / 0.16
  wide, PyTorch element-wise   41    1.2e-6 / 1.5e-6    9.4e-6 / 1.2e-5    1.0e-6 / 1.8e-6    0.17 / 0.16
  float64 (limit 1e-10): K14 general form 2.9e-15 / 1.6e-14 over 323 cases, K12 6.9e-15 / 1.6e-14 over 13.
No kernel bug was found: under these metrics the kernels are as close to float64 as eager float32 autograd is.
"""
import numpy as np
import pytest
import torch

from tests import gradient_checks as gc

pytestmark = pytest.mark.gpu

ROWS_SHAPES = [(3, 256, 2), (2, 512, 4), (5, 256, 6), (3, 768, 8), (2, 512, 10), (1, 256, 10), (2, 512, 12), (2, 768, 14)]
RAGGED_SHAPES = [(2, 513, 5, 3), (3, 300, 12, 2), (1, 1000, 3, 7), (5, 64, 16, 16), (4, 1, 1, 1)]
LOGWEIGHT_SHAPES = [(3, 700, 10, 10), (2, 513, 5, 3), (7, 300, 12, 2), (2, 2048, 8, 8)]
WIDE_SHAPES = [(2, 320, 128, 128), (2, 96, 256, 256), (1, 320, 192, 80), (2, 512, 64, 48), (2, 1000, 24, 24)]
# rows of 128 values on both sides in whole tiles of 256 particles: the shapes at which the element-wise parts of the wide
# backward are the hand-written passes (aesmc_wide_adjoint_scale / _merge) and not PyTorch's operations
WIDE_FUSED_SHAPES = [(2, 512, 128, 128), (3, 1024, 128, 128)]
ROUTES = ["plain", "ancestors", "children", "ancestors_and_children"]
VARIANTS = [(weights, with_grad_x) for weights in ("flat", "probes", "probes_last_row") for with_grad_x in (False, True)]
ROWS_FORM, GENERAL_FORM = 2, 1


@pytest.fixture(scope="module")
def kernels(hip_device):
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


@pytest.fixture
def step_form(kernels):
    """Chooses K14's form and grid for one test; the default again afterwards."""
    lib = kernels._lib

    def choose(form, grid=0):
        assert lib.aesmc_test_set_step_backward(form, grid) == 0
    yield choose
    lib.aesmc_test_set_step_backward(0, 0)


def _report(family, dtype, what, mine, reference, limits, draw=0):
    print("FIGURES family={} dtype={} case={} draw={} e_ref_particle={:.3e} e_ref_reduced={:.3e} limit_particle={:.3e} "
          "limit_reduced={:.3e} err_particle={:.3e} err_reduced={:.3e} slots={}".format(
              family, str(dtype).replace("torch.", ""), what.replace(" ", "_"), draw,
              reference["particle"] if reference else 0.0, reference["reduced"] if reference else 0.0, limits[0], limits[1],
              mine["particle"], mine["reduced"], ",".join("{}:{:.1e}".format(*item) for item in mine["slots"].items())))


def _weights(kind, B, K, dtype, device, seed):
    """(lw, lse, grad_lse, rows with particles that count) for one regime."""
    gen = torch.Generator().manual_seed(seed)
    grad_lse = torch.randn(B, generator=gen, dtype=torch.float64).to(dtype).to(device)
    if kind == "flat":
        lw, lse = gc.flat_weights(B, K, dtype, device, seed)
        return lw, lse, grad_lse, torch.ones(B, dtype=torch.bool, device=device)
    lw, lse, has = gc.probe_weights(B, K, dtype, device, rows=None if kind == "probes" else [B - 1])
    return lw, lse, torch.where(has, grad_lse, torch.zeros_like(grad_lse)), has


def _float32_term(lw, lse, grad_lse):
    return grad_lse.unsqueeze(1) * torch.exp(lw - lse.unsqueeze(1))


def _assert_silent_rows(got, has, arrives, what):
    """Rows of the batch without a particle that counts: y's gradient exactly zero; the proposal offset's too unless a
    gradient arrives at x_t from later steps."""
    if bool(has.all()):
        return
    assert bool((got[2][~has] == 0).all()), what + ": y's gradient in a row without probes"
    if not arrives:
        assert bool((got[8][~has] == 0).all()), what + ": off_q's gradient in a row without probes"


class _Step:
    """One step's operands and everything that may reach it, for one route."""

    def __init__(self, kernels, shape, dtype, device, route, seed, matched=False, wide=False):
        B, K, dx, dy = shape
        self.shape, self.dtype, self.device, self.kernels = shape, dtype, device, kernels
        if wide:
            self.o = gc.step_operands(B, K, dx, dy, dtype, device, seed, matched=matched, spread=0.3 / np.sqrt(dx),
                                      emission=1.0 / np.sqrt(dx))
        else:
            self.o = gc.step_operands(B, K, dx, dy, dtype, device, seed, matched=matched)
        o = self.o
        self.ancestors = None
        if route in ("ancestors", "ancestors_and_children"):
            self.ancestors = gc.sorted_indices(B, K, seed + 1, device)
        elif route == "children":      # the children's ranges are taken through ancestors only: everybody its own
            self.ancestors = torch.arange(K, device=device).repeat(B, 1)
        self.next_ancestors = self.child_end = None
        if route in ("children", "ancestors_and_children"):
            self.next_ancestors = gc.sorted_indices(B, K, seed + 2, device)
            self.child_end = gc.child_ranges(self.next_ancestors)
        self.terms = ((o["A"], o["off_p"]), (o["C"], o["off_g"]), (o["Q"], o["off_q"]))
        self.scales = (o["s_p"], o["s_g"], o["s_q"])
        self.x = gc.draw(o, self.ancestors)
        self.seed = seed

    def arriving(self, with_grad_x):
        """(kernel arguments, the summed gradient at x_t in float64, the same in the operands' dtype) or Nones."""
        extra, total64, total = {}, None, None
        if self.ancestors is not None:
            extra["ancestors"] = self.ancestors
        if with_grad_x:
            extra["grad_x"] = gc.arriving_gradient(self.o, self.seed + 3)
            total64, total = extra["grad_x"].double(), extra["grad_x"]
        if self.child_end is not None:
            extra["child_grad"] = gc.arriving_gradient(self.o, self.seed + 4, index=self.next_ancestors)
            extra["child_end"] = self.child_end
            summed64 = gc.sum_children(extra["child_grad"], self.next_ancestors)
            summed = gc.sum_children(extra["child_grad"], self.next_ancestors, dtype=self.dtype)
            total64 = summed64 if total64 is None else total64 + summed64
            total = summed if total is None else total + summed
        return extra, total64, total

    def own_weights(self):
        """The forward launches' own log-weights of x_t (and x_t as THEY draw it) — flat, or the case is not one."""
        k, o = self.kernels, self.o
        moved = o["x_prev"] if self.ancestors is None else k.gather(o["x_prev"], self.ancestors)
        self.x = k.affine_rsample(moved, o["Q"], o["off_q"], o["eps"], o["s_q"])
        lw = k.affine_logweight(moved, self.x, o["y"], *self.terms, self.scales)
        lse = k.logweight_lse(lw, None, None, want_lw=False)[1]
        gc.assert_flat(lw)
        return lw, lse

    def references(self, lw, lse, grad_lse, total64, total):
        g = gc.softmax_term(lw, lse, grad_lse)
        self.g = g
        self.cancellation = lambda: gc.step_scale_cancellation(self.o, self.x, g, total64, self.ancestors)
        want = gc.step_reference(self.o, self.x, g, total64, self.ancestors)
        scales = {0: gc.step_particle_scale(self.o, self.x, g, total64, self.ancestors)}
        stand_in = None
        if self.dtype == torch.float32:
            stand_in = gc.step_reference(self.o, self.x, _float32_term(lw, lse, grad_lse), total, self.ancestors,
                                         dtype=torch.float32)
        return want, scales, stand_in


NEED_STEP = [True, False] + [True] * 10


def _declines(K):
    """The general kernel takes a tile of 256 particles that spans at most 8 batch rows."""
    return 255 // K + 2 > 8


DRAWS = 8      # inputs on which eager float32 autograd is itself ill-conditioned are drawn again, at most so often


def _run_step_variants(kernels, make_step, family, expect_form, variants=VARIANTS, natural=False, expect_per_lane=1):
    """`make_step(draw)` -> the _Step of that draw (another seed for each)."""
    lib = kernels._lib
    real_unfused = kernels.affine_step_backward_unfused
    unfused = {"calls": 0}

    def counting(*args, **kwargs):
        unfused["calls"] += 1
        return real_unfused(*args, **kwargs)
    kernels.affine_step_backward_unfused = counting
    try:
        for kind, with_grad_x in variants:
            for draw in range(DRAWS):
                step = make_step(draw)
                B, K, dx, dy = step.shape
                if kind == "probes_last_row" and B == 1:
                    break
                if natural:
                    lw, lse = step.own_weights()
                    grad_lse, has = _weights("flat", B, K, step.dtype, step.device, step.seed + 5)[2:]
                else:
                    lw, lse, grad_lse, has = _weights(kind, B, K, step.dtype, step.device, step.seed + 5)
                extra, total64, total = step.arriving(with_grad_x)
                want, scales, stand_in = step.references(lw, lse, grad_lse, total64, total)
                if stand_in is None or gc.well_conditioned(stand_in, want, scales, step.g, step.cancellation):
                    break
            else:
                raise AssertionError("{} {} {}: none of {} draws of the inputs is well-conditioned".format(
                    family, step.shape, kind, DRAWS))
            if kind == "probes_last_row" and B == 1:
                continue
            what = "{} {} {}{}".format(family, "x".join(map(str, step.shape)), kind, " grad_x" if with_grad_x else "")
            before = unfused["calls"]
            got = kernels.affine_step_backward(step.o["x_prev"], step.x, step.o["y"], *step.terms, step.scales, NEED_STEP,
                                               lw, lse, grad_lse=grad_lse, **extra)
            torch.cuda.synchronize()
            assert got[1] is None
            assert unfused["calls"] - before == (1 if _declines(K) else 0), what + ": the route taken"
            if step.dtype == torch.float32:      # (float64 has the general kernel only: no form is recorded for it)
                assert lib.aesmc_test_last_step_backward_form() == expect_form, what + ": the form that ran"
            # (a declined shape reads 0 — K14's launch, then K12's inside the unfused route, both decline it)
            assert lib.aesmc_test_last_affine_backward_particles_per_lane() == (0 if _declines(K) else expect_per_lane), \
                what + ": particles per lane"
            figures = gc.check(got, want, scales, stand_in=stand_in, what=what)
            _report(family, step.dtype, what, *figures, draw=draw)
            _assert_silent_rows(got, has, total64 is not None, what)
            assert kernels.read_flags(step.device) == 0
    finally:
        del kernels.affine_step_backward_unfused


# ---- K14, rows form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", ROWS_SHAPES)
def test_rows_form_gives_every_particle_its_gradient(kernels, hip_device, step_form, shape, route):
    B, K, d = shape
    step_form(0)
    make = lambda draw: _Step(kernels, (B, K, d, d), torch.float32, hip_device, route, seed=17 * B + K + d + 1000 * draw)
    _run_step_variants(kernels, make, "K14-rows", ROWS_FORM)


@pytest.mark.parametrize("route", ROUTES)
def test_rows_form_carries_its_sums_from_tile_to_tile(kernels, hip_device, step_form, route):
    """Sixteen tiles on three workgroups: five or six tiles each, of two different batch rows."""
    step_form(0, grid=3)
    make = lambda draw: _Step(kernels, (4, 1024, 10, 10), torch.float32, hip_device, route, seed=23 + 1000 * draw)
    _run_step_variants(kernels, make, "K14-rows", ROWS_FORM)


# ---- K14, general form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", [(B, K, d, d) for B, K, d in ROWS_SHAPES] + [(4, 1024, 10, 10)] + RAGGED_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_general_form_gives_every_particle_its_gradient(kernels, hip_device, step_form, shape, route, dtype):
    B, K, dx, dy = shape
    step_form(1, grid=3 if K == 1024 else 0)
    make = lambda draw: _Step(kernels, shape, dtype, hip_device, route, seed=13 * B + K + dx + dy + 1000 * draw)
    _run_step_variants(kernels, make, "K14-general", GENERAL_FORM)


@pytest.mark.parametrize("route", ["plain", "ancestors_and_children"])
def test_general_form_with_two_particles_per_lane(kernels, hip_device, step_form, route):
    """Latent rows of 10 and observation rows of 11 float32 values at 2^20 particles: where the step's general kernel gives
    a lane two particles — the extents pad to 12 (rows padded to 10 and below always get one particle per lane), there
    are 2^20 particles (fewer always get one), and three tiles of 512 such rows still fit the 78 KiB of LDS that two
    workgroups per compute unit leave each (rows of 11 or 12 latent values do not, and fall back to one)."""
    step_form(1)
    make = lambda draw: _Step(kernels, (256, 4096, 10, 11), torch.float32, hip_device, route, seed=29 + 1000 * draw)
    _run_step_variants(kernels, make, "K14-general-two-per-lane", GENERAL_FORM,
                       variants=[("flat", True), ("probes_last_row", False)], expect_per_lane=2)


@pytest.mark.parametrize("form,shape", [(0, (2, 512, 10, 10)), (1, (2, 513, 5, 3)), (1, (2, 512, 12, 12))])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_step_backward_on_the_forward_launches_own_weights(kernels, hip_device, step_form, form, shape, dtype):
    """Transition equal to proposal, a weak emission: the log-weights K10 computes are themselves flat (asserted).  With a
    gradient arriving at x_t only: on this model x_t - loc_p does not depend on x_{t-1}, so without one a particle's
    gradient is what is left after two terms fifty times its size cancel, and float32 autograd is itself 2e-5 off."""
    if dtype == torch.float64 and form == 0:
        form = 1      # (no rows form in float64)
    step_form(form)
    make = lambda draw: _Step(kernels, shape, dtype, hip_device, "ancestors", seed=31 + 1000 * draw, matched=True)
    _run_step_variants(kernels, make, "K14-own-weights", ROWS_FORM if form == 0 else GENERAL_FORM,
                       variants=[("flat", True)], natural=True)


# ---- two chained steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1], ids=["rows", "general"])
def test_two_chained_steps_finish_both_steps_parameter_gradients(kernels, hip_device, step_form, form):
    """The later step defers, the earlier carries: A, C, Q and the scales come back once, as the sum over both steps —
    against float64 autograd over both; everything per step (x_prev's rows, y, the offsets) against its own step's."""
    step_form(form)
    lib = kernels._lib
    shape = (2, 512, 10, 10)
    B, K, dx, dy = shape
    shared = ("A", "C", "Q", "s_p", "s_g", "s_q")
    steps = []
    for number in range(2):
        step = _Step(kernels, shape, torch.float32, hip_device, "ancestors", seed=41 + 10 * number)
        if number == 1:
            for name in shared + ("off_p", "off_g"):
                step.o[name] = steps[0].o[name]
            step.terms = ((step.o["A"], step.o["off_p"]), (step.o["C"], step.o["off_g"]), (step.o["Q"], step.o["off_q"]))
            step.scales = steps[0].scales
            step.x = gc.draw(step.o, step.ancestors)
        lw, lse, grad_lse, _ = _weights("flat", B, K, torch.float32, hip_device, step.seed + 5)
        extra, total64, total = step.arriving(True)
        step.call = lambda chain, step=step, lw=lw, lse=lse, grad_lse=grad_lse, extra=extra: kernels.affine_step_backward(
            step.o["x_prev"], step.x, step.o["y"], *step.terms, step.scales, NEED_STEP, lw, lse, grad_lse=grad_lse,
            chain=chain, **extra)
        step.want, step.particle_scales, step.stand_in = step.references(lw, lse, grad_lse, total64, total)
        steps.append(step)
    earlier, later = steps
    expect = ROWS_FORM if form == 0 else GENERAL_FORM
    chain = {"carry": None, "defer": True}
    deferred = later.call(chain)
    assert lib.aesmc_test_last_step_backward_form() == expect
    left = chain["left"]
    assert left is not None and left[1] >= 1
    slots = [gc.SLOTS.index(name) for name in shared]
    assert all(deferred[slot] is None for slot in slots)
    per_step = lambda values: [None if slot in slots else value for slot, value in enumerate(values)]
    figures = gc.check(deferred, per_step(later.want), later.particle_scales, stand_in=per_step(later.stand_in),
                       what="the deferring step")
    _report("K14-chain", torch.float32, "deferring", *figures)
    chain = {"carry": left, "defer": False}
    carried = earlier.call(chain)
    assert lib.aesmc_test_last_step_backward_form() == expect and chain["left"] is None
    both = lambda a, b: [u if slot not in slots else u + v for slot, (u, v) in enumerate(zip(a, b))]
    figures = gc.check(carried, both(earlier.want, later.want), earlier.particle_scales,
                       stand_in=both(earlier.stand_in, later.stand_in), what="the carrying step")
    _report("K14-chain", torch.float32, "carrying", *figures)
    assert kernels.read_flags(hip_device) == 0


# ---- K12 ----------------------------------------------------------------------------------------------------------------------
def _run_logweight_variants(kernels, shape, dtype, device, seed, variants, matched=False, family="K12", expect_per_lane=1):
    B, K, dx, dy = shape
    real_unfused = kernels.affine_logweight_backward_unfused
    unfused = {"calls": 0}

    def counting(*args, **kwargs):
        unfused["calls"] += 1
        return real_unfused(*args, **kwargs)
    kernels.affine_logweight_backward_unfused = counting
    try:
        for kind in variants:
            if kind == "probes_last_row" and B == 1:
                continue
            what = "{} {} {}".format(family, "x".join(map(str, shape)), kind)
            for draw in range(DRAWS):
                o = gc.step_operands(B, K, dx, dy, dtype, device, seed + 1000 * draw, matched=matched)
                terms = ((o["A"], o["off_p"]), (o["C"], o["off_g"]), (o["Q"], o["off_q"]))
                scales = (o["s_p"], o["s_g"], o["s_q"])
                # x_t is a leaf here and any value will do: noise of scale 0.9 — an exact draw from the proposal (or, for the
                # matched model, from the transition) makes that scale's gradient a sum of terms of mean zero
                x = gc.draw(o, noise_scale=0.9)
                if kind == "own":
                    lw = kernels.affine_logweight(o["x_prev"], x, o["y"], *terms, scales)
                    lse = kernels.logweight_lse(lw, None, None, want_lw=False)[1]
                    gc.assert_flat(lw)
                    grad_lse, has = _weights("flat", B, K, dtype, device, seed + 5)[2:]
                else:
                    lw, lse, grad_lse, has = _weights(kind, B, K, dtype, device, seed + 5)
                g = gc.softmax_term(lw, lse, grad_lse)
                want = gc.log_weight_reference(o, x, g)
                particle_scales = gc.log_weight_particle_scales(o, x, g)
                stand_in = None
                if dtype == torch.float32:
                    stand_in = gc.log_weight_reference(o, x, _float32_term(lw, lse, grad_lse), dtype=torch.float32)
                if stand_in is None or gc.well_conditioned(stand_in, want, particle_scales, g,
                                                           lambda: gc.log_weight_scale_cancellation(o, x, g)):
                    break
            else:
                raise AssertionError("{}: none of {} draws of the inputs is well-conditioned".format(what, DRAWS))
            got = kernels.affine_logweight_backward(o["x_prev"], x, o["y"], *terms, scales, [True] * 12, lw=lw, lse=lse,
                                                    grad_lse=grad_lse)
            torch.cuda.synchronize()
            assert unfused["calls"] == 0, what + ": K12 declined the shape"      # (it has one form)
            assert kernels._lib.aesmc_test_last_affine_backward_particles_per_lane() == expect_per_lane, \
                what + ": particles per lane"
            figures = gc.check(got, want, particle_scales, stand_in=stand_in, what=what)
            _report(family, dtype, what, *figures, draw=draw)
            _assert_silent_rows(got, has, False, what)
    finally:
        del kernels.affine_logweight_backward_unfused


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape", LOGWEIGHT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_logweight_backward_gives_every_particle_its_gradient(kernels, hip_device, shape, dtype):
    _run_logweight_variants(kernels, shape, dtype, hip_device, seed=sum(shape), variants=["flat", "probes", "probes_last_row"])


def test_logweight_backward_with_two_particles_per_lane(kernels, hip_device):
    """2^20 float32 particles: K12 gives a lane two of them from there on."""
    _run_logweight_variants(kernels, (256, 4096, 10, 10), torch.float32, hip_device, seed=37,
                            variants=["flat", "probes_last_row"], family="K12-two-per-lane", expect_per_lane=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_logweight_backward_on_the_forward_launches_own_weights(kernels, hip_device, dtype):
    _run_logweight_variants(kernels, (3, 700, 10, 10), dtype, hip_device, seed=43, variants=["own"], matched=True,
                            family="K12-own-weights")


# ---- the wide backward --------------------------------------------------------------------------------------------------------
def _run_wide_variants(kernels, make_step, variants, family="wide", natural=False):
    counts = {"wide": 0, "scale": 0, "merge": 0}
    real_wide, real_scale, real_merge = kernels.affine_step_backward_wide, kernels.wide_adjoint_scale, kernels.wide_adjoint_merge

    def counting(name, real):
        def call(*args, **kwargs):
            counts[name] += 1
            return real(*args, **kwargs)
        return call
    kernels.affine_step_backward_wide = counting("wide", real_wide)
    kernels.wide_adjoint_scale = counting("scale", real_scale)
    kernels.wide_adjoint_merge = counting("merge", real_merge)
    try:
        for kind, with_grad_x in variants:
            for draw in range(DRAWS):
                step = make_step(draw)
                B, K, dx, dy = step.shape
                if natural:
                    o = step.o
                    out_x = torch.empty_like(o["x_prev"])
                    lw = kernels.affine_propagate_wide(o["x_prev"], o["eps"], o["y"], *step.terms, step.scales, out_x,
                                                       ancestors=step.ancestors)
                    assert lw is not None, "the wide forward launch declined the shape"
                    step.x = out_x
                    gc.assert_flat(lw)
                    lse = torch.logsumexp(lw, dim=1)
                    grad_lse, has = _weights("flat", B, K, step.dtype, step.device, step.seed + 5)[2:]
                else:
                    lw, lse, grad_lse, has = _weights(kind, B, K, step.dtype, step.device, step.seed + 5)
                extra, total64, total = step.arriving(with_grad_x)
                want, scales, stand_in = step.references(lw, lse, grad_lse, total64, total)
                if gc.well_conditioned(stand_in, want, scales, step.g, step.cancellation):
                    break
            else:
                raise AssertionError("{} {} {}: none of {} draws of the inputs is well-conditioned".format(
                    family, step.shape, kind, DRAWS))
            what = "{} {} {}{}{}".format(family, "x".join(map(str, step.shape)), kind, " grad_x" if with_grad_x else "",
                                         " ancestors" if step.ancestors is not None else "")
            # the hand-written passes take whole tiles of rows of `wide_dim` float32 values on both sides: stated per shape,
            # so that a change of the tile or of the conditions cannot quietly leave them out of every case
            fused = tuple(step.shape) in WIDE_FUSED_SHAPES
            assert fused == (dx == dy == kernels.wide_dim and K % kernels.wide_adjoint_tile == 0), what
            before = dict(counts)
            got = kernels.affine_step_backward(step.o["x_prev"], step.x, step.o["y"], *step.terms, step.scales, NEED_STEP,
                                               lw, lse, grad_lse=grad_lse, **extra)
            torch.cuda.synchronize()
            assert got[1] is None
            assert counts["wide"] - before["wide"] == 1, what + ": not the wide backward"
            assert counts["scale"] - before["scale"] == (1 if fused else 0), what + ": the emission's fused pass"
            assert counts["merge"] - before["merge"] == (1 if fused else 0), what + ": the transition's fused pass"
            figures = gc.check(got, want, scales, stand_in=stand_in, what=what)
            _report(family + ("-fused" if fused else ""), step.dtype, what, *figures, draw=draw)
            _assert_silent_rows(got, has, total64 is not None, what)
    finally:
        del kernels.affine_step_backward_wide, kernels.wide_adjoint_scale, kernels.wide_adjoint_merge


@pytest.mark.parametrize("route", ["plain", "ancestors"])
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_backward_gives_every_particle_its_gradient(kernels, hip_device, shape, route):
    """The recomputing adjoint where its element-wise parts are PyTorch's operations (widths other than 128, or K not in
    whole tiles of 256).  A gradient of order 1 arrives at x_t (the other wide test's 1e-3 randn lay below its own
    tolerance); the probes once without it, where every other particle's row has to be exactly zero."""
    make = lambda draw: _Step(kernels, shape, torch.float32, hip_device, route, seed=sum(shape) + 1000 * draw, wide=True)
    _run_wide_variants(kernels, make, [("flat", True), ("probes", True), ("probes_last_row", True), ("probes", False)])


@pytest.mark.parametrize("route", ["plain", "ancestors"])
@pytest.mark.parametrize("shape", WIDE_FUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_backward_through_its_fused_passes_gives_every_particle_its_gradient(kernels, hip_device, shape, route):
    """Rows of 128 values in whole tiles: aesmc_wide_adjoint_scale (the emission's adjoint in place, sum d^2 per particle,
    the row sums behind y's and off_g's gradients) and aesmc_wide_adjoint_merge (the transition's, what arrives at x_t
    merged in — `grad_x` handed in as the kernel's `add` operand, and absent —, the row sums behind off_p's and off_q's)
    each run once per case (counted): two and four tiles per batch row, so a row's sums are put together from several."""
    make = lambda draw: _Step(kernels, shape, torch.float32, hip_device, route, seed=sum(shape) + 1000 * draw, wide=True)
    _run_wide_variants(kernels, make, [("flat", True), ("flat", False), ("probes", True), ("probes", False),
                                       ("probes_last_row", True), ("probes_last_row", False)])


def test_wide_backward_on_the_forward_launches_own_weights(kernels, hip_device):
    """Rows of 24 values: there the matched model's own log-weights (K17g / K18g) are flat; at 128 values no model of
    this kind keeps them so, which is why the cases above hand the weights in."""
    make = lambda draw: _Step(kernels, (2, 1000, 24, 24), torch.float32, hip_device, "ancestors", seed=47 + 1000 * draw,
                              matched=True, wide=True)
    _run_wide_variants(kernels, make, [("flat", True)], family="wide-own-weights", natural=True)
