"""tests/proposal_net_checks.py can fail: eager float32 CPU autograd of b2 + W2 tanh(c1 + W1 x) stands in for kernel K13b,
passes as it is, and fails once a fault the kernel could plausibly have is planted in its output.  Every fault's
docstring records what the metric of test_particle_mlp_backward_equals_float64_autograd (max norm over the tensor's
largest entry, float32 limit 6e-5) reads for it at the three shapes below, flat upstream: the structural faults and the
flushed derivative are seen by both, a tanh that is 1e-5 off passes the earlier metric at every shape.
"""
import pytest
import torch

from tests import gradient_checks as gc
from tests import proposal_net_checks as pn

SHAPES = [(3, 768, 10, 64, 10), (2, 512, 5, 16, 3), (2, 256, 8, 17, 8)]
CPU = torch.device("cpu")


class _Case:
    def __init__(self, shape, regime):
        B, K, din, H, dout = shape
        self.shape, self.regime = shape, regime
        self.o = pn.operands(B, K, din, H, dout, torch.float32, CPU, seed=B * K + H)
        self.G = pn.upstream(regime, B, K, dout, torch.float32, CPU, seed=K + dout)
        self.want = pn.reference(self.o, self.G)
        self.scales = pn.scales(self.o, self.G, self.want)
        self.stand_in = pn.stand_in(self.o, self.G)

    def planted(self):
        return {name: self.stand_in[name].clone() for name in ("x", "W1", "c1", "W2")}

    def restated(self, h=None, factor=None):
        """The gradients written out in float64 — with another `h` or another factor in place of 1 - h^2 —, rounded."""
        o, G = self.o, self.G.double()
        h = self.want["h"] if h is None else h
        factor = 1.0 - h * h if factor is None else factor
        dh = torch.matmul(G, o["W2"].double()) * factor
        got = {"x": torch.matmul(dh, o["W1"].double()), "W1": torch.einsum("bkh,bki->hi", dh, o["x"].double()),
               "c1": dh.sum(dim=1), "W2": torch.einsum("bko,bkh->oh", G, h)}
        return {name: value.float() for name, value in got.items()}

    def terms(self, b, k):
        """(g [dout], h [H], dh [H]) of particle (b, k) in float32."""
        g = self.G[b, k]
        h = self.want["h"][b, k].float()
        return g, h, (g @ self.o["W2"]) * (1.0 - h * h)


@pytest.fixture(scope="module", params=[(shape, regime) for shape in SHAPES for regime in ("flat", "probes")],
                ids=lambda p: "{}-{}".format("x".join(map(str, p[0])), p[1]))
def case(request):
    return _Case(*request.param)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def flat_case(request):
    return _Case(request.param, "flat")


def _fails(case, got, what):
    print("{} at {} {}: the earlier metric reads {:.2e}".format(what, case.shape, case.regime,
                                                                 pn.earlier_metric(got, case.want)))
    with pytest.raises(AssertionError):
        pn.check(got, case.want, case.scales, stand_in_grads=case.stand_in)


def _a_counted_particle(case, b):
    """The particle of batch row `b` with the smallest nonzero scale."""
    A = case.scales["x"][b]
    return int(torch.where(A > 0, A, torch.full_like(A, float("inf"))).argmin())


def test_eager_float32_autograd_passes_its_own_limit(case):
    mine, reference, allowed = pn.check(case.planted(), case.want, case.scales, stand_in_grads=case.stand_in)
    print("stand-in at {} {}: {}".format(case.shape, case.regime, mine))
    # (a sum over B K = 2304 particles: 5.7e-7 .. 1.8e-6 off depending on the order the CPU's matmul adds them in)
    assert max(allowed.values()) <= gc.CONDITION_LIMIT and min(allowed.values()) >= 16 * gc.EPS32
    assert pn.earlier_metric(case.planted(), case.want) <= 6e-5


@pytest.mark.parametrize("shape", [(1, 256, 1, 1, 1), (5, 256, 15, 33, 16)], ids=lambda s: "x".join(map(str, s)))
def test_eager_float32_autograd_passes_at_the_smallest_and_the_widest_net(shape):
    for regime in pn.REGIMES[:2]:
        c = _Case(shape, regime)
        mine, _, _ = pn.check(c.planted(), c.want, c.scales, stand_in_grads=c.stand_in)
        print("stand-in at {} {}: {}".format(shape, regime, mine))


def test_restated_gradients_pass(case):
    """The float64 restatement the tanh faults are planted in is itself right."""
    pn.check(case.restated(), case.want, case.scales, stand_in_grads=case.stand_in)


def test_a_particle_whose_gradient_was_not_written_fails(case):
    """The grad_x row of the particle with the smallest scale of its batch row left at zero: 1.0 per particle.  Earlier
    metric (flat): 1.2e-1, 5.0e-2, 3.9e-2."""
    got = case.planted()
    k = _a_counted_particle(case, 0)
    got["x"][0, k] = 0.0
    _fails(case, got, "a row never written")
    err, _ = gc.particle_error(got["x"], case.want["x"], case.scales["x"])
    assert 0.0 < err <= 1.01


def test_a_particle_left_out_of_the_second_layers_gradient_fails(case):
    """One particle missing from grad_W2 = sum g (x) h.  Earlier metric (flat): 1.2e-2, 3.1e-2, 3.6e-2."""
    got = case.planted()
    b = case.shape[0] - 1
    g, h, _ = case.terms(b, gc.probe_positions(case.shape[1])[1])
    got["W2"] -= torch.outer(g, h)
    _fails(case, got, "a particle left out of grad_W2")


def test_a_particle_added_twice_to_the_second_layers_gradient_fails(case):
    """The same particle counted twice.  Earlier metric (flat): 1.2e-2, 3.1e-2, 3.6e-2."""
    got = case.planted()
    b = case.shape[0] - 1
    g, h, _ = case.terms(b, gc.probe_positions(case.shape[1])[1])
    got["W2"] += torch.outer(g, h)
    _fails(case, got, "a particle twice in grad_W2")


def test_a_wavefronts_row_sum_credited_to_the_next_batch_row_fails(case):
    """The sum of dh over the last 64 particles of batch row 0 (a tile's last wavefront) added to row 1's grad_c1
    instead.  Earlier metric (flat): 1.6e-1, 6.4e-1, 5.8e-1; with probes one particle moves (K - 1): 3.7e-1, 5.4e-1, 3.1e-1."""
    got = case.planted()
    K = case.shape[1]
    moved = sum(case.terms(0, k)[2] for k in range(K - 64, K))
    assert float(moved.abs().max()) > 0
    got["c1"][0] -= moved
    got["c1"][1] += moved
    _fails(case, got, "a wavefront's row sum in the wrong row")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] > 16], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("regime", ["flat", "probes"])
def test_a_chunk_of_hidden_units_missing_from_one_particle_fails(shape, regime):
    """Hidden units 16 .. 31 (the second chunk) missing from one particle's grad_x.  Earlier metric (flat): 2.8e-1 at 64
    hidden units; 4.7e-3 at 17, where the chunk holds one unit."""
    c = _Case(shape, regime)
    got = c.planted()
    k = gc.probe_positions(shape[1])[2]
    dh = c.terms(0, k)[2]
    got["x"][0, k] -= dh[16:32] @ c.o["W1"][16:32]
    _fails(c, got, "a chunk of hidden units missing")


def test_a_tanh_that_is_1e_5_off_fails(case):
    """h = tanh z + 1e-5 in both uses (the outer product and 1 - h^2).  Earlier metric: 2.6e-5, 3.6e-5, 2.2e-5
    (flat) and 2.5e-5, 3.2e-5, 2.7e-5 (probes) — all below its 6e-5 limit.  Here grad_x reads 1.8e-5 .. 8.8e-5 per particle
    against limits of 1.9e-6 .. 2.0e-6, grad_c1 1.4e-5 .. 3.5e-5 against 1.9e-6 .. 2.0e-6."""
    got = case.restated(h=case.want["h"] + 1e-5)
    earlier = pn.earlier_metric(got, case.want)
    _fails(case, got, "tanh 1e-5 off")
    assert earlier <= 6e-5, "the earlier metric is not expected to see this fault"


def test_a_flushed_derivative_fails(flat_case):
    """1 - h^2 taken as 0 where |z| > 4 (1.3e-3 there at most).  Earlier metric (flat): 3.2e-4, 5.2e-4, 3.6e-4 — five to nine
    times its limit, where a missing particle is a thousand times it; per particle the fault reads 3.3e-4 .. 1.5e-3, two
    to seven hundred times the limit."""
    case = flat_case
    z, h = case.want["z"], case.want["h"]
    reached = (z.abs() > 4) & (pn.reach(case.o, case.G) > 0)
    assert bool(reached.any()), "no pre-activation beyond 4 in this draw"
    got = case.restated(factor=torch.where(z.abs() > 4, torch.zeros_like(h), 1.0 - h * h))
    _fails(case, got, "1 - h^2 flushed")
