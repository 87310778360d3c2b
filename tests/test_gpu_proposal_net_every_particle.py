"""The proposal net's kernels (K13 forward, K13b backward: out = b2 + W2 tanh(c1[b] + W1 x)) against float64 with EVERY
particle counting, in the layouts the model passes, on saturated pre-activations, and the float32 path end to end.

The earlier K13b test (test_gpu_linear_gaussian.py::test_particle_mlp_backward_equals_float64_autograd) compares every
output in a max norm relative to the tensor's largest entry and allows float32 6e-5: a recomputed tanh that is 1e-5 off
passes it at every shape (tests/test_proposal_net_checks.py).  Here the metrics and limits are those of
tests/proposal_net_checks.py: grad_x particle by particle against the absolute sum of the particle's own terms, grad_c1
batch row by batch row, the contracted gradients relative to their largest entry without a floor, the forward element
by element against |b2| + sum |W2| |h|; float32 limit max(8 e_ref, 16 eps32 = 1.9e-6) with e_ref the error of eager
float32 PyTorch on the device on the same inputs under the same metric, float64 limit 1e-10.  Every case asserts that
the kernel ran (the provider returned a result, the device status word is 0).

Families:
  * K13b at the smallest shapes at which each mechanism is in play (BACKWARD_SHAPES), upstream flat / at probes / at the
    last batch row's probes, with and without grad_x (the other outputs bit for bit the same), twice around a freed
    block of NaNs (bit for bit the same); one float32 case in which workgroups walk two tiles;
  * layouts: W1 a column slice, W2 a transposed view, x a slice and a [K,B,din] transpose, the upstream expanded from one
    element and from [B,1,dout], c1 as [H], [B,H] and an expanded row — bit for bit the dense call;
  * saturation: c1 shifted by +-4, +-9, +-20, +-1e4, one batch row by 20 (float64: 40) or more in every unit — forward
    under its metric, backward under A' (proposal_net_checks), grad_x exactly zero in the saturated row;
  * the recomputed tanh read back through grad_W2 (W1 = 0, one-hot upstream rows) on 0, +-1e-4, +-0.5, a grid on
    [-12, 12], +-20, +-88, +-1e4;
  * K13 at 43 particles per row (a tile spanning seven batch rows), at its own edge (37: eight rows, all the offset table
    holds) and ragged shapes, with and without b2, c1 [H] and [B,H], against float64 and the C oracle; K = 36 is
    declined and the operator gives PyTorch's numbers (K = 42 is NOT declined: `particle_mlp_covers` asks for
    255 // K + 2 <= 8, so 42 runs the kernel and is checked like the rest);
  * the operator `particle_mlp` in float32, all five leaves;
  * NonlinearSsm(fused=True) in float32 against a float64 copy, draws replayed, ancestors equal at every step: value and
    every parameter's gradient at most max(2 x the plain float32 model's error, 16 eps32) off.

Measured on an MI355X, the worst over the family's cases and outputs (every case prints a FIGURES line: e_ref / limit /
error per output; the last column is the output that came closest to its own limit):

  family (float32)            cases   worst e_ref   largest limit   worst error   error / limit
  K13b                          23      7.4e-7         5.9e-6          4.0e-6        0.97  (1x256x1x1x1 flat, grad_x)
  K13b, two tiles                2      3.2e-6         2.6e-5          4.2e-7        0.15
  saturated, backward            2      9.3e-7         7.5e-6          8.4e-7        0.16
  saturated, forward             2      5.5e-8         1.9e-6          1.5e-7        0.08
  the recomputed tanh            1      3.8e-8         4.8e-7          1.7e-7        0.35  (at z = -2.75)
  K13                           36      1.1e-5         8.6e-5          3.2e-7        0.17
  operator, gradients            4      6.1e-7         4.8e-6          4.8e-7        0.25
  operator, forward              4      2.1e-7         1.9e-6          2.1e-7        0.11
  fused model (seed 0)          11      7.5e-7         1.9e-6          6.3e-7        0.33
  float64 (limit 1e-10): K13b 1.9e-15 over 23 cases, saturated 2.4e-15 / 4.0e-16, tanh 5.6e-17, K13 1.0e-12 over 36.

No kernel or binder bug was found.  Two things the figures show.  The hardware exp2 / rcp tanh of float32 K13b is 1.7e-7
off at worst (the library's, torch.tanh, 3.8e-8) and exactly +-1 from |z| = 20 on, as its comment claims; at the net of one
hidden unit, where a particle's gradient is a single term w1 (1 - h^2) t, that difference is the whole of the kernel's
4.0e-6 against eager autograd's 5.2e-7: inside the limit, by 3 %.  Next come grad_x at 3x256x3x7x2 and 2x512x5x16x3, flat,
1.6e-6 at 0.78 and 0.72 of their limits; every other output of every case is below 0.4 of its own.  (K13's largest
e_ref, 1.1e-5, is eager PyTorch at the one-unit net without b2: it rounds W1 x before adding c1, the kernel's fused chain
does not and is 1.4e-7 off there.)
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import gradient_checks as gc
from tests import proposal_net_checks as pn

pytestmark = pytest.mark.gpu

# (B, K, din, H, dout): DP is the padded row of max(din, dout) values (4, 8, 10, 12, 16), a chunk 16 hidden units
BACKWARD_SHAPES = [(1, 256, 1, 1, 1),        # DP 4, one chunk nearly all padding
                   (3, 256, 3, 7, 2),        # tile = batch row
                   (2, 512, 5, 16, 3),       # DP 8, H exactly one chunk
                   (2, 256, 8, 17, 8),       # the second chunk holds one unit
                   (3, 768, 10, 64, 10),     # DP 10, four chunks
                   (2, 512, 12, 48, 9),      # DP 12
                   (5, 256, 15, 33, 16),     # DP 16, the ones column beside 15 inputs, dout 16
                   (2, 256, 2, 64, 16)]      # dout > din
FORWARD_SHAPES = [(9, 43, 10, 64, 10),       # seven batch rows per tile, partial last tile
                  (1, 43, 3, 7, 2), (7, 64, 3, 7, 7), (3, 257, 5, 16, 3), (2, 300, 15, 33, 16), (1, 1000, 10, 48, 4),
                  (4, 256, 1, 1, 1),
                  (9, 42, 10, 64, 10),       # still covered: 255 // K + 2 <= 8 holds down to K = 37
                  (9, 37, 10, 64, 10)]       # the edge itself: a tile spans eight batch rows of the offset table
DTYPES = [torch.float32, torch.float64]
DTYPE_IDS = ["float32", "float64"]
_name = lambda shape: "x".join(map(str, shape))
_short = lambda dtype: str(dtype).replace("torch.", "")


@pytest.fixture(scope="module")
def kernels(hip_device):
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _report(family, dtype, what, errors, reference, allowed):
    outputs = " ".join("{}={:.3e}/{:.3e}/{:.3e}".format(name, reference[name] if reference else 0.0, allowed[name], err)
                       for name, err in errors.items() if name != "silent")
    print("FIGURES family={} dtype={} case={} (e_ref/limit/error) {}".format(family, _short(dtype), what.replace(" ", "_"),
                                                                            outputs))


def _report_one(family, dtype, what, err, e_ref, limit):
    _report(family, dtype, what, {"out": err}, None if e_ref is None else {"out": e_ref}, {"out": limit})


def _backward(kernels, G, o, need_x=True):
    got = kernels.particle_mlp_backward(G, o["x"], o["W1"], o["c1"], o["W2"], need_x=need_x)
    assert got is not None, "K13b declined a shape it is built for"
    torch.cuda.synchronize()
    assert kernels.read_flags(G.device) == 0
    return dict(zip(("x", "W1", "c1", "W2"), got))


def _forward(kernels, o, with_b2=True):
    out = kernels.particle_mlp(o["x"], o["W1"], o["c1"], o["W2"], o["b2"] if with_b2 else None)
    assert out is not None, "K13 declined a shape it is built for"
    torch.cuda.synchronize()
    assert kernels.read_flags(out.device) == 0
    return out


def _same_bits(a, b, what):
    for name in b:
        if b[name] is None:
            assert a[name] is None, what + ": " + name
        else:
            assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), what + ": " + name


def _free_a_block_of_nans(kernels, o, G):
    """Blocks of the sizes the binder asks for (grad_x, the two record areas, the rows' sums), filled with NaN and freed:
    the caching allocator hands them to the next call."""
    B, K, din = o["x"].shape
    chunks = (o["W1"].size(0) + 15) // 16
    records = int(kernels._lib.aesmc_particle_mlp_backward_records(B, K))
    sizes = [B * K * din, records * chunks * 256, records * chunks * 256, B * (K // 64) * 16 * chunks, 1 << 20]
    blocks = [torch.full((n,), float("nan"), dtype=G.dtype, device=G.device) for n in sizes]
    torch.cuda.synchronize()
    del blocks


# ---- K13b ----------------------------------------------------------------------------------------------------------------------
def _check_backward(kernels, shape, dtype, device, regime, seed, family="K13b"):
    B, K, din, H, dout = shape
    what = "{} {} {}".format(family, _name(shape), regime)
    o = pn.operands(B, K, din, H, dout, dtype, device, seed)
    G = pn.upstream(regime, B, K, dout, dtype, device, seed + 1)
    want = pn.reference(o, G)
    sc = pn.scales(o, G, want)
    stand_in = pn.stand_in(o, G) if dtype == torch.float32 else None
    got = _backward(kernels, G, o)
    _report(family, dtype, what, *pn.check(got, want, sc, stand_in, what=what))
    if regime == "probes_last_row":
        assert bool((got["c1"][:B - 1] == 0).all()) and bool((got["x"][:B - 1] == 0).all()), what + ": rows nothing reaches"
    lean = _backward(kernels, G, o, need_x=False)
    assert lean["x"] is None
    _same_bits(lean, dict(got, x=None), what + " without grad_x")
    _free_a_block_of_nans(kernels, o, G)
    _same_bits(_backward(kernels, G, o), got, what + " after a freed block of NaNs")


# The seed is 7 B + K + H but for the net of ONE hidden unit: there a particle's gradient has a single term, w1 (1 - h^2) t, and
# at the seed the rule gives (264) pre-activations reach 3.7, where float32 holds 1 - h^2 to 1e-4 only and eager autograd is
# 1.7e-5 off under the per-particle metric (8 e_ref > 1e-4: ill-conditioned).  Seed 269 keeps |z| below 2.4.
SEEDS = {(1, 256, 1, 1, 1): 269}

# (with one batch row the last row's probes are the probes: no third case there)
BACKWARD_CASES = [(shape, regime) for shape in BACKWARD_SHAPES for regime in pn.REGIMES
                  if not (regime == "probes_last_row" and shape[0] == 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape,regime", BACKWARD_CASES, ids=lambda v: _name(v) if isinstance(v, tuple) else v)
def test_backward_gives_every_particle_its_gradient(kernels, hip_device, shape, regime, dtype):
    _check_backward(kernels, shape, dtype, hip_device, regime, seed=SEEDS.get(shape, 7 * shape[0] + shape[1] + shape[3]))


@pytest.mark.parametrize("regime", ["flat", "probes_last_row"])
def test_backward_where_a_workgroup_walks_two_tiles(kernels, hip_device, regime):
    """The matrix accumulators of a wavefront carry over from its first tile to its second while column 15 — the rows'
    sums — is handed out and cleared per tile: the smallest K (a multiple of 256) at which, with B = 3, there are more
    wavefronts' worth of particles than records plus 32, i.e. at least nine workgroups take a second tile."""
    records = lambda K: int(kernels._lib.aesmc_particle_mlp_backward_records(3, K))
    K = 256
    while not 3 * K // 64 > records(K) + 32:
        K += 256
        assert K <= 1 << 18
    assert 3 * K / 64 > records(K) + 32 and K % 256 == 0
    _check_backward(kernels, (3, K, 10, 64, 10), torch.float32, hip_device, regime, seed=61, family="K13b-two-tiles")


# ---- layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_layouts_the_model_passes_give_the_dense_calls_bits(kernels, hip_device, dtype):
    B, K, din, H, dout, dy = 3, 512, 6, 24, 4, 5
    o = pn.operands(B, K, din, H, dout, dtype, hip_device, seed=71)
    G = pn.upstream("flat", B, K, dout, dtype, hip_device, seed=72)
    junk = lambda *shape: torch.randn(*shape, dtype=dtype, device=hip_device)

    def both(o_, G_):
        return dict(_backward(kernels, G_, o_), out=_forward(kernels, o_))

    dense = both(o, G)
    want = pn.reference(o, G)
    pn.check({name: value for name, value in dense.items() if name != "out"}, want, pn.scales(o, G, want),
             pn.stand_in(o, G) if dtype == torch.float32 else None, what="layouts, the dense call")
    views = {
        "W1 a column slice of [H, din + dy]": dict(W1=torch.cat([o["W1"], junk(H, dy)], dim=1)[:, :din]),
        "W2 a transposed view": dict(W2=o["W2"].t().contiguous().t()),
        "x a slice of a wider tensor": dict(x=torch.cat([o["x"], junk(B, K, 3)], dim=2)[:, :, :din]),
        "x a [K,B,din] transpose": dict(x=o["x"].transpose(0, 1).contiguous().transpose(0, 1)),
    }
    for what, replaced in views.items():
        (name, view), = replaced.items()
        assert not view.is_contiguous() and torch.equal(view, o[name]), what
        _same_bits(both(dict(o, **replaced), G), dense, what)
    # the upstream of `.sum().backward()` (one element, stride 0 everywhere) and of a sum over the particles
    for what, source in (("upstream expanded from one element", junk(1, 1, 1)),
                         ("upstream expanded from [B,1,dout]", junk(B, 1, dout))):
        view = source.expand(B, K, dout)
        assert 0 in view.stride()
        _same_bits(_backward(kernels, view, o), _backward(kernels, view.contiguous(), o), what)
    # one offset for every batch row: as [H], as a [1,H] row expanded to [B,H], and written out as [B,H]
    row = o["c1"][:1]
    written = dict(o, c1=row.expand(B, H).contiguous())
    want = both(written, G)
    _same_bits(both(dict(o, c1=row.expand(B, H)), G), want, "c1 a [1,H] row expanded to [B,H]")
    _same_bits(both(dict(o, c1=row[0].clone()), G), want, "c1 as [H]")


# ---- saturation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", [(3, 512, 10, 64, 10), (2, 256, 5, 16, 3)], ids=_name)
def test_saturated_hidden_units(kernels, hip_device, shape, dtype):
    """Finite inputs only.  (float64: the library's tanh is exactly 1 beyond 19.06 only, so the saturated row is shifted by
    40 or more there — the pre-activations scatter by several units around the shift.)"""
    B, K, din, H, dout = shape
    what = "saturated {}".format(_name(shape))
    o = pn.saturate(pn.operands(B, K, din, H, dout, dtype, hip_device, seed=81 + H), fully_saturated_row=B - 1,
                    at_least=20.0 if dtype == torch.float32 else 40.0)
    G = pn.upstream("flat", B, K, dout, dtype, hip_device, seed=82)
    want = pn.reference(o, G, with_b2=True)
    assert float(want["z"][B - 1].abs().min()) > (9.5 if dtype == torch.float32 else 19.5)
    assert all(bool(torch.isfinite(t).all()) for t in list(o.values()) + [G])
    stand_in = pn.stand_in(o, G, with_b2=True) if dtype == torch.float32 else None
    out = _forward(kernels, o)
    _report_one("saturated-forward", dtype, what, *pn.check_forward(out, want, o, None if stand_in is None else
                                                                    stand_in["out"], what=what))
    got = _backward(kernels, G, o)
    assert all(bool(torch.isfinite(t).all()) for t in got.values()), what
    _report("saturated-backward", dtype, what, *pn.check(got, want, pn.scales(o, G, want, saturated=True), stand_in,
                                                         what=what))
    assert bool((got["x"][B - 1] == 0).all()), what + ": grad_x in the fully saturated row"


# ---- the recomputed tanh -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_the_recomputed_tanh_read_back_through_the_second_layers_gradient(kernels, hip_device, dtype):
    """W1 = 0, so z = c1; batch row b has ONE particle with an upstream, 1 at output b: grad_W2[b, :] is the kernel's own
    tanh(c1[b, :]) — one product by 1 and sums with exact zeros."""
    B = H = dout = 16
    K, din = 256, 3
    special = [0.0, 1e-4, -1e-4, 0.5, -0.5, 20.0, -20.0, 88.0, -88.0, 1e4, -1e4]
    z = torch.cat([torch.tensor(special, dtype=torch.float64),
                   torch.linspace(-12.0, 12.0, B * H - len(special), dtype=torch.float64)]).to(dtype)
    o = pn.operands(B, K, din, H, dout, dtype, hip_device, seed=91)
    o["W1"] = torch.zeros_like(o["W1"])
    o["c1"] = z.reshape(B, H).to(hip_device)
    G = torch.zeros(B, K, dout, dtype=dtype, device=hip_device)
    probes = gc.probe_positions(K)
    for b in range(B):
        G[b, probes[b % len(probes)], b] = 1.0
    h = _backward(kernels, G, o)["W2"].double().cpu().reshape(-1)
    z64 = z.double()
    want = torch.tanh(z64)
    err = float((h - want).abs().max())
    if dtype == torch.float32:
        e_ref = float((torch.tanh(z.to(hip_device)).double().cpu() - want).abs().max())
        limit = max(8.0 * e_ref, 4.0 * gc.EPS32)
    else:
        e_ref, limit = None, gc.FLOAT64_TOLERANCE
    at = int((h - want).abs().argmax())
    print("the recomputed tanh, {}: largest error {:.3e} at z = {:.6g}".format(_short(dtype), err, float(z64[at])))
    _report_one("tanh", dtype, "the recomputed tanh", err, e_ref, limit)
    assert err <= limit, (err, limit, float(z64[at]))
    far = z64.abs() >= 20
    assert int(far.sum()) == 6 and bool((h[far] == torch.sign(z64[far])).all()), h[far]
    assert float(h[0]) == 0.0


# ---- K13 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=_name)
def test_forward_element_by_element(kernels, hip_device, shape, dtype):
    B, K, din, H, dout = shape
    for shared in (False, True):
        o = pn.operands(B, K, din, H, dout, dtype, hip_device, seed=3 * B + K + H, shared_offset=shared)
        G = torch.zeros(B, K, dout, dtype=dtype, device=hip_device)
        want = pn.reference(o, G, with_b2=True)
        for with_b2 in (True, False):
            what = "K13 {} c1 {} {}".format(_name(shape), "[H]" if shared else "[B,H]", "b2" if with_b2 else "no b2")
            reference = dict(want, out=want["out"] if with_b2 else want["out"] - o["b2"].double())
            stand_in = None
            if dtype == torch.float32:
                stand_in = pn.expression(o["x"], o["W1"], o["c1"], o["W2"], o["b2"] if with_b2 else None)
            out = _forward(kernels, o, with_b2)
            assert out.shape == (B, K, dout) and out.dtype == dtype
            _report_one("K13", dtype, what, *pn.check_forward(out, reference, o, stand_in, with_b2=with_b2, what=what))
            # the C oracle: the same fma chains, libm's tanh against the device's (a few ulp)
            host = {name: value.cpu().numpy() for name, value in o.items()}
            oracle = c_oracle.particle_mlp(host["x"], host["W1"], host["c1"], host["W2"], host["b2"] if with_b2 else None)
            tolerance = 3e-6 if dtype == torch.float32 else 1e-14
            np.testing.assert_allclose(out.cpu().numpy(), oracle, rtol=tolerance, atol=4 * tolerance)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_too_short_for_the_offset_table_are_declined(kernels, hip_device, dtype):
    """A tile of 256 particles may span 255 // K + 2 batch rows, and the table of the rows' offsets holds eight: K = 37 is
    the last size covered ("about 43" in the binder's words; 42 and 37 run the kernel in the test above), K = 36 the first
    that `particle_mlp_covers` turns down — there the operator gives the PyTorch expression's own numbers."""
    from aesmc_amd.linear_gaussian import particle_mlp
    o = pn.operands(9, 36, 10, 64, 10, dtype, hip_device, seed=5)
    args = (o["x"], o["W1"], o["c1"], o["W2"], o["b2"])
    for K in (37, 42, 43):
        assert kernels.particle_mlp_covers(*pn.operands(9, K, 10, 64, 10, dtype, hip_device, seed=5).values()), K
    assert not kernels.particle_mlp_covers(*args) and kernels.particle_mlp(*args) is None
    assert torch.equal(particle_mlp(*args), pn.expression(*args))
    assert kernels.read_flags(hip_device) == 0


# ---- the operator --------------------------------------------------------------------------------------------------------------
class _counting:
    """Counts the provider's K13 / K13b calls that returned a result."""

    def __init__(self, provider):
        self.provider, self.count = provider, {"forward": 0, "backward": 0}

    def __enter__(self):
        forward, backward = self.provider.particle_mlp, self.provider.particle_mlp_backward

        def spy(name, real):
            def call(*args, **kwargs):
                out = real(*args, **kwargs)
                self.count[name] += out is not None
                return out
            return call
        self.provider.particle_mlp, self.provider.particle_mlp_backward = spy("forward", forward), spy("backward", backward)
        return self

    def __exit__(self, *exc):
        del self.provider.particle_mlp, self.provider.particle_mlp_backward
        return False


@pytest.mark.parametrize("shared", [False, True], ids=["c1_per_row", "c1_shared"])
@pytest.mark.parametrize("regime", ["flat", "probes_last_row"])
def test_the_operator_in_float32_binds_every_gradient(kernels, hip_device, shared, regime):
    """`linear_gaussian.particle_mlp`, all five leaves: _ParticleMlp.backward's binding of the rows' sums (kept per row, or
    added over the rows for a shared offset) and of the bias."""
    from aesmc_amd.linear_gaussian import particle_mlp
    B, K, din, H, dout = 3, 512, 6, 20, 4
    what = "operator c1 {} {}".format("[H]" if shared else "[B,H]", regime)
    o = pn.operands(B, K, din, H, dout, torch.float32, hip_device, seed=101, shared_offset=shared)
    G = pn.upstream(regime, B, K, dout, torch.float32, hip_device, seed=102)
    want = pn.reference(o, G, with_b2=True)
    stand_in = pn.stand_in(o, G, with_b2=True)
    leaves = {name: o[name].clone().requires_grad_(True) for name in pn.NAMES}
    with _counting(kernels) as calls:
        out = particle_mlp(*[leaves[name] for name in pn.NAMES])
        grads = torch.autograd.grad(out, [leaves[name] for name in pn.NAMES], G)
    torch.cuda.synchronize()
    assert calls.count == {"forward": 1, "backward": 1} and kernels.read_flags(hip_device) == 0
    got = dict(zip(pn.NAMES, grads))
    assert all(got[name].shape == o[name].shape for name in pn.NAMES)
    _report_one("operator-forward", torch.float32, what, *pn.check_forward(out.detach(), want, o, stand_in["out"], what=what))
    _report("operator", torch.float32, what, *pn.check(got, want, pn.scales(o, G, want), stand_in, what=what))


# ---- the whole fused model -------------------------------------------------------------------------------------------------------
def _value_and_gradients(model, observations, K):
    from aesmc_amd import inference
    result = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                             return_log_marginal_likelihood=True, return_latents=False, return_log_weight=False,
                             return_ancestral_indices=True)
    value = result["log_marginal_likelihood"].mean()
    value.backward()
    grads = {name: p.grad.detach() for name, p in model.named_parameters() if p.grad is not None}
    return value.detach(), grads, [a.cpu() for a in result["ancestral_indices"]]


def test_the_fused_nonlinear_model_in_float32_is_as_close_to_float64_as_the_plain_one(kernels, hip_device):
    """NonlinearSsm(5, hidden=24) at B = 2, K = 256, T = 3: the plain float32 model on the device records its draws; the
    fused float32 model (K8, K13 / K13b) and a float64 copy of the plain one replay them.  On the first seed at which
    all three resample the same ancestors at every step, the fused run's value and parameter gradients are at most
    max(2 x the plain run's error, 16 eps32) from float64's."""
    from aesmc_amd.testing import models, replay
    d, B, K, T = 5, 2, 256, 3
    for seed in range(8):
        plain = models.NonlinearSsm(d, hidden=24, seed=0, dtype=torch.float32).to(hip_device)
        fused = models.NonlinearSsm(d, hidden=24, seed=0, dtype=torch.float32, fused=True).to(hip_device)
        exact = models.NonlinearSsm(d, hidden=24, seed=0, dtype=torch.float32).to(hip_device).double()
        assert all(torch.equal(p.float(), q) for p, q in zip(exact.parameters(), plain.parameters()))
        observations = plain.simulate(T, B, seed=1)
        np.random.seed(seed)
        torch.manual_seed(seed)
        with replay.record() as tape:
            plain_run = _value_and_gradients(plain, observations, K)
        with replay.replay(tape), _counting(kernels) as calls:
            fused_run = _value_and_gradients(fused, observations, K)
        with replay.replay(tape):
            exact_run = _value_and_gradients(exact, [y.double() for y in observations], K)
        if all(torch.equal(a, c) and torch.equal(b, c) for a, b, c in zip(plain_run[2], fused_run[2], exact_run[2])):
            break
    else:
        raise AssertionError("no seed in range(8) at which the three runs resample the same ancestors")
    print("the fused nonlinear model: seed {}".format(seed))
    assert len(exact_run[2]) == T - 1
    assert calls.count == {"forward": T - 1, "backward": T - 1}, calls.count
    assert kernels.read_flags(hip_device) == 0
    assert sorted(fused_run[1]) == sorted(plain_run[1]) == sorted(exact_run[1]) and any(n.startswith("net.") for n in exact_run[1])
    figures = {"value": (gc.reduced_error(plain_run[0], exact_run[0]), gc.reduced_error(fused_run[0], exact_run[0]))}
    for name, want in exact_run[1].items():
        figures[name] = (gc.reduced_error(plain_run[1][name], want), gc.reduced_error(fused_run[1][name], want))
    for name, (e_plain, e_fused) in figures.items():
        limit = max(2.0 * e_plain, 16.0 * gc.EPS32)
        print("FIGURES family=model dtype=float32 case={} (e_ref/limit/error) out={:.3e}/{:.3e}/{:.3e}".format(
            name, e_plain, limit, e_fused))
    for name, (e_plain, e_fused) in figures.items():
        assert e_fused <= max(2.0 * e_plain, 16.0 * gc.EPS32), (name, e_fused, e_plain)
