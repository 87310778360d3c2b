"""The item form of the fused propagation launch (linear_gaussian_item.hip; aesmc/inference.py:102-126 with state.py:98,
:179 for a linear-Gaussian model) where it works on wavefront-uniform operands:

  * its table of per-batch-row vectors (the three offsets and the observation) is fetched through one buffer descriptor
    per vector, built by scalar arithmetic — absent vectors, strided observations, windows that straddle two batch rows,
    a window whose second row lies beyond the batch and partial last windows must give what the other forms give;
  * with the densities' constants behind the weight pairs (aesmc_affine_weight_pairs_scaled) the three divisions by
    2 s^2 go through reciprocals formed once per workgroup, behind a guard; pairs without constants
    (aesmc_affine_weight_pairs) keep the plain divisions — the two launches must agree bit for bit, also where the
    guard sends a wavefront back to the divisions (an overflowing sum of squares, a sum that is exactly zero).

References: the launch with untagged pairs, the persistent form (above 12 values per row: the first form) through the
test hook, and the log-weight kernel over `philox_normal_fill` noise — the compositions the other suites already pin.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_linear_gaussian import operands
from tests.test_gpu_noise_and_lazy_latents import _ancestors

pytestmark = pytest.mark.gpu

PERSISTENT, ITEM = 1, 2


@pytest.fixture(scope="module")
def kernels(hip_device):
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


@pytest.fixture()
def forms(kernels):
    lib = kernels._lib
    yield lambda form: lib.aesmc_test_set_k16_form(form)
    lib.aesmc_test_set_k16_form(0)


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _launch(kernels, x_prev, idx, y, terms, scales, tagged, seed):
    """aesmc_affine_normal_propagate_drawn_paired with pairs that carry the constants (`tagged`) or not; returns x_t, the
    log-weights and the form that ran."""
    from aesmc_amd import _philox
    from aesmc_amd._kernels import _ptr
    dev = x_prev.device
    B, K, dx = x_prev.shape
    maps = [kernels._affine_map(*term) for term in terms]
    pairs = kernels._build_pairs(maps, list(scales) if tagged else None, dev)
    tag = int(pairs[-2:-1].view(torch.int32).item())
    assert tag == ((0x5c000000 | (terms[1][0].shape[0] << 8) | dx) if tagged else 0)
    torch.manual_seed(seed)
    reservation = _philox.reserve(B * K * dx, dev)
    out_x = torch.full_like(x_prev, float("nan"))
    lw = torch.full((B, K), float("nan"), device=dev)
    status = kernels._lib.aesmc_affine_normal_propagate_drawn_paired(
        _ptr(x_prev), _ptr(idx), _ptr(y), y.stride(0), ctypes.byref(maps[0][0]), ctypes.byref(maps[1][0]),
        ctypes.byref(maps[2][0]), _ptr(scales[0]), _ptr(scales[1]), _ptr(scales[2]), _ptr(out_x), _ptr(lw),
        _ptr(kernels.flags(dev)), B, K, reservation.seed, reservation.offset, reservation.threads,
        _ptr(reservation.state), _ptr(pairs), kernels._stream(x_prev))
    assert status == 0
    return out_x, lw, kernels._lib.aesmc_test_last_k16_form(), reservation


def _inputs(shape, device, gather, y_pad=0):
    B, K, dx, dy = shape
    _, o = operands(2, 8, dx, dy, np.float32, device, seed=B + K + dx)
    gen = torch.Generator(device=device).manual_seed(K + dx + dy)
    x_prev = torch.randn(B, K, dx, device=device, generator=gen)
    y = torch.randn(B, dy + y_pad, device=device, generator=gen)[:, :dy]      # (a row stride larger than dy when padded)
    off_p = torch.randn(dx, device=device, generator=gen)                     # shared by every batch row
    off_q = torch.randn(B, dx, device=device, generator=gen)                  # one per batch row
    off_g = torch.randn(B, dy, device=device, generator=gen)
    idx = _ancestors(B, K, device, seed=B + K, spread=1.0) if gather else None
    return o, x_prev, y, off_p, off_q, off_g, idx


def _check_against_every_reference(kernels, forms, x_prev, idx, y, terms, scales, seed):
    dev = x_prev.device
    kernels.read_flags(dev)
    forms(ITEM)
    got_x, got_lw, ran, reservation = _launch(kernels, x_prev, idx, y, terms, scales, True, seed)
    assert ran == ITEM, "the item form declined a shape it is built for"
    plain_x, plain_lw, ran, _ = _launch(kernels, x_prev, idx, y, terms, scales, False, seed)
    assert ran == ITEM
    assert _same(got_x, plain_x) and _same(got_lw, plain_lw), "tagged and untagged constants disagree"
    forms(PERSISTENT)
    want_x, want_lw, ran, _ = _launch(kernels, x_prev, idx, y, terms, scales, True, seed)
    assert ran == PERSISTENT
    assert _same(got_x, want_x) and _same(got_lw, want_lw), "the item form and the persistent form disagree"
    forms(0)
    eps = kernels.philox_normal(reservation, tuple(x_prev.shape), dev)
    k15_x = torch.full_like(x_prev, float("nan"))
    k15_lw = kernels.affine_propagate(x_prev, eps, y, *terms, scales, out_x=k15_x, ancestors=idx)
    assert k15_lw is not None
    assert _same(got_x, k15_x) and _same(got_lw, k15_lw), "the item form and fill + the log-weight kernel disagree"
    assert torch.isfinite(got_lw).all() and kernels.read_flags(dev) == 0


# windows straddle two batch rows, the last window is partial and a window's second row falls beyond the batch (B = 3 with
# K = 192, 320); every kind of row (pairs, quads, dwords; 13 .. 16 values); compile-time and run-time observation extents
SHAPES = [(3, 192, 10, 10), (3, 320, 10, 10), (3, 320, 2, 1), (2, 320, 3, 7), (4, 1024, 16, 16), (3, 192, 10, 16)]


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_tagged_constants_give_the_plain_divisions_bits(kernels, hip_device, forms, shape, gather):
    o, x_prev, y, off_p, off_q, off_g, idx = _inputs(shape, hip_device, gather)
    terms = ((o["A"], off_p), (o["C"], off_g), (o["Q"], off_q))
    _check_against_every_reference(kernels, forms, x_prev, idx, y, terms, (o["s_p"], o["s_g"], o["s_q"]), seed=11 + shape[1])


@pytest.mark.parametrize("absent", ["p", "g", "q", "pgq"])
@pytest.mark.parametrize("shape", [(3, 320, 10, 10), (3, 192, 3, 7)])
def test_absent_offset_vectors_are_zeros(kernels, hip_device, forms, shape, absent):
    o, x_prev, y, off_p, off_q, off_g, idx = _inputs(shape, hip_device, True)
    terms = ((o["A"], None if "p" in absent else off_p), (o["C"], None if "g" in absent else off_g),
             (o["Q"], None if "q" in absent else off_q))
    _check_against_every_reference(kernels, forms, x_prev, idx, y, terms, (o["s_p"], o["s_g"], o["s_q"]), seed=5)
    # and an absent vector is the vector of zeros, bit for bit
    zeros = ((o["A"], torch.zeros_like(off_p) if "p" in absent else off_p),
             (o["C"], torch.zeros_like(off_g) if "g" in absent else off_g),
             (o["Q"], torch.zeros_like(off_q) if "q" in absent else off_q))
    forms(ITEM)
    a = _launch(kernels, x_prev, idx, y, terms, (o["s_p"], o["s_g"], o["s_q"]), True, 5)
    b = _launch(kernels, x_prev, idx, y, zeros, (o["s_p"], o["s_g"], o["s_q"]), True, 5)
    assert a[2] == ITEM and b[2] == ITEM and _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("shape", [(3, 320, 10, 10), (3, 192, 10, 16), (2, 320, 3, 7)])
def test_an_observation_with_a_row_stride_larger_than_its_extent(kernels, hip_device, forms, shape):
    o, x_prev, y, off_p, off_q, off_g, idx = _inputs(shape, hip_device, True, y_pad=5)
    assert y.stride(0) == shape[3] + 5 and y.stride(1) == 1
    terms = ((o["A"], off_p), (o["C"], off_g), (o["Q"], off_q))
    _check_against_every_reference(kernels, forms, x_prev, idx, y, terms, (o["s_p"], o["s_g"], o["s_q"]), seed=23)
    forms(ITEM)
    dense = _launch(kernels, x_prev, idx, y.contiguous(), terms, (o["s_p"], o["s_g"], o["s_q"]), True, 23)
    strided = _launch(kernels, x_prev, idx, y, terms, (o["s_p"], o["s_g"], o["s_q"]), True, 23)
    assert _same(dense[0], strided[0]) and _same(dense[1], strided[1])


@pytest.mark.parametrize("case", ["overflow", "zero"])
@pytest.mark.parametrize("K", [192, 320])
def test_the_guard_sends_a_wavefront_back_to_the_divisions(kernels, hip_device, forms, case, K):
    """A sum of squares outside the guard in some lanes only — one batch row whose x_{t-1} is 1e20 (the transition's sum
    overflows), one batch row whose observation equals the emission's location exactly (C = 0, g = 0, y = 0: the sum
    is +0 and the quotient -0) — gives the untagged launch's bits, infinities and zero signs included."""
    shape = (3, K, 10, 10)
    o, x_prev, y, off_p, off_q, off_g, idx = _inputs(shape, hip_device, False)
    C = o["C"]
    if case == "overflow":
        x_prev = x_prev.clone()
        x_prev[1] = 1e20
    else:
        C, off_g, y = torch.zeros_like(C), torch.zeros_like(off_g), y.clone()
        y[1] = 0.0
    terms = ((o["A"], off_p), (C, off_g), (o["Q"], off_q))
    scales = (o["s_p"], o["s_g"], o["s_q"])
    forms(ITEM)
    got_x, got_lw, ran, _ = _launch(kernels, x_prev, None, y, terms, scales, True, 31)
    assert ran == ITEM
    want_x, want_lw, ran, _ = _launch(kernels, x_prev, None, y, terms, scales, False, 31)
    assert ran == ITEM
    assert _same(got_x, want_x) and _same(got_lw, want_lw)
    if case == "overflow":
        assert not torch.isfinite(got_lw[1]).any() and torch.isfinite(got_lw[0]).all() and torch.isfinite(got_lw[2]).all()
    else:
        assert torch.isfinite(got_lw).all()
    kernels.read_flags(hip_device)
