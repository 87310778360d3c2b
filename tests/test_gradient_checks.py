"""tests/gradient_checks.py can fail: eager float32 CPU autograd stands in for a kernel on the flat inputs, passes as it
is, and fails once a fault a kernel could plausibly have is planted in its output.  The first of them — one particle's
gradient never written — is 1.0 under the per-particle metric and 2e-5 .. 9e-5 under the floored max norm the backward
tests used before: below that norm's 3e-5 limit at (2, 513, 5, 3), two or three times above it at the other shapes — a
margin of rounding, not of structure.  And no test module defines a test twice.
"""
import ast
import glob
import os

import pytest
import torch

from tests import gradient_checks as gc

SHAPES = [(2, 512, 10, 10), (3, 256, 2, 2), (2, 768, 14, 14), (2, 513, 5, 3)]
CPU = torch.device("cpu")


class _Case:
    """One step on flat weights: the float64 reference, the per-particle scale and the float32 stand-in's output."""

    def __init__(self, shape, with_grad_x):
        B, K, dx, dy = shape
        self.shape = shape
        self.operands = gc.step_operands(B, K, dx, dy, torch.float32, CPU, seed=B * K + dx)
        self.x = gc.draw(self.operands)
        self.lw, self.lse = gc.flat_weights(B, K, torch.float32, CPU, seed=K + dy)
        gen = torch.Generator().manual_seed(7)
        self.grad_lse = torch.randn(B, generator=gen)
        self.grad_x = gc.arriving_gradient(self.operands, seed=11) if with_grad_x else None
        self.g = gc.softmax_term(self.lw, self.lse, self.grad_lse)
        self.want = gc.step_reference(self.operands, self.x, self.g, self.grad_x)
        self.scales = {0: gc.step_particle_scale(self.operands, self.x, self.g, self.grad_x)}
        g32 = self.grad_lse.unsqueeze(1) * torch.exp(self.lw - self.lse.unsqueeze(1))
        self.stand_in = gc.step_reference(self.operands, self.x, g32, self.grad_x, dtype=torch.float32)

    def planted(self):
        return [None if t is None else t.clone() for t in self.stand_in]

    def only(self, b, k):
        """The float32 gradients of particle (b, k) alone."""
        g = torch.zeros_like(self.g)
        g[b, k] = self.g[b, k]
        return gc.step_reference(self.operands, self.x, g, None, dtype=torch.float32)


@pytest.fixture(scope="module", params=[(shape, with_grad_x) for shape in SHAPES for with_grad_x in (False, True)],
                ids=lambda p: "{}-{}".format("x".join(map(str, p[0])), "grad_x" if p[1] else "elbo_only"))
def case(request):
    return _Case(*request.param)


def _fails(case, got):
    with pytest.raises(AssertionError):
        gc.check(got, case.want, case.scales, stand_in=case.stand_in)


def test_eager_float32_autograd_passes_and_sets_a_limit_near_1e_5(case):
    mine, reference, limits = gc.check(case.stand_in, case.want, case.scales, stand_in=case.stand_in)
    print("stand-in at {}: per-particle {:.2e}, reduced {:.2e}".format(case.shape, mine["particle"], mine["reduced"]))
    assert max(limits) <= 5e-5 and min(limits) >= 16 * gc.EPS32


def test_a_particle_whose_gradient_was_not_written_fails(case):
    """(a) the x_prev gradient of the lowest-weight particle of a row zeroed: 1.0 under the per-particle metric."""
    got = case.planted()
    k = int(case.lw[0].argmin())
    got[0][0, k] = 0.0
    _fails(case, got)
    err, _ = gc.particle_error(got[0], case.want[0], case.scales[0])
    assert 0.99 <= err <= 1.01
    if case.grad_x is None:
        # what the tests asked before: the max norm over all particles, floored at 1, against 3e-5 — an error of order
        # 1 in this particle is four orders smaller there, and at the ragged shape it passes outright
        floored = float((got[0].double() - case.want[0]).abs().max()) / max(1.0, float(case.want[0].abs().max()))
        print("floored max norm of the same fault at {}: {:.2e}".format(case.shape, floored))
        assert floored < 1e-3
        if case.shape == (2, 513, 5, 3):
            assert floored <= 3e-5


@pytest.mark.parametrize("which", ["lowest weight", "median weight"])
def test_a_particle_left_out_of_a_weight_gradient_fails(case, which):
    """(b) one particle missing from A's gradient."""
    got = case.planted()
    order = case.lw[1].argsort()
    k = int(order[0] if which == "lowest weight" else order[len(order) // 2])
    got[3] -= case.only(1, k)[3]
    _fails(case, got)


def test_an_offset_gradient_written_to_the_wrong_row_fails(case):
    """(c) row 0's off_q gradient written to row 1."""
    got = case.planted()
    got[8][1] = got[8][0]
    _fails(case, got)


def test_two_particles_swapped_fail(case):
    """(d) the last particle of a row swapped with its neighbour."""
    got = case.planted()
    K = case.shape[1]
    got[0][-1, [K - 2, K - 1]] = got[0][-1, [K - 1, K - 2]]
    _fails(case, got)


def test_probe_weights_leave_only_the_probes():
    lw, lse, has = gc.probe_weights(3, 700, torch.float32, CPU, rows=[2])
    g = gc.softmax_term(lw, lse, torch.where(has, torch.ones(3), torch.zeros(3)))
    probes = gc.probe_positions(700)
    assert probes == [0, 63, 64, 255, 256, 699] and gc.probe_positions(64) == [0, 63] and gc.probe_positions(1) == [0]
    assert int((g != 0).sum()) == len(probes) and bool((g[2, probes] > 0).all()) and float(g[:2].abs().max()) == 0.0
    torch.testing.assert_close(g[2, probes], torch.full((len(probes),), 1.0 / len(probes), dtype=torch.float64),
                               rtol=1e-6, atol=0)
    with pytest.raises(AssertionError):
        gc.assert_flat(lw)


def test_child_ranges_and_sums_follow_the_next_steps_ancestors():
    index = gc.sorted_indices(3, 40, seed=1, device=CPU)
    assert bool((index[:, 1:] >= index[:, :-1]).all()) and bool((index[-1] == 40 // 3).all())
    ends = gc.child_ranges(index)
    assert ends.dtype == torch.int32 and bool((ends[:, -1] == 40).all())
    rows = torch.randn(3, 40, 2, dtype=torch.float64)
    summed = gc.sum_children(rows, index)
    for b in range(3):
        start = 0
        for k in range(40):
            torch.testing.assert_close(summed[b, k], rows[b, start:int(ends[b, k])].sum(0), rtol=1e-12, atol=1e-12)
            start = int(ends[b, k])


def test_no_test_module_defines_a_test_twice():
    """A second top-level `def test_x` replaces the first silently: the first is never collected."""
    here = os.path.dirname(os.path.abspath(__file__))
    repeated = []
    for path in sorted(glob.glob(os.path.join(here, "*.py"))):
        with open(path) as source:
            tree = ast.parse(source.read(), filename=path)
        seen = {}
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name.startswith("test_"):
                if node.name in seen:
                    repeated.append("{}: {} (lines {} and {})".format(os.path.basename(path), node.name, seen[node.name],
                                                                      node.lineno))
                seen[node.name] = node.lineno
    assert not repeated, repeated
