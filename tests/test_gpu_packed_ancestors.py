"""The resampling hand-off as one 32-bit word per particle (aesmc/inference.py:234-269 produces the indices; state.py:179
and its backward consume them): aesmc_resample_step_packed writes  idx | child_end << 16, K16
(aesmc_affine_normal_propagate_drawn_packed) and K14's rows form (aesmc_affine_step_backward_packed) read the words as
they are, aesmc_unpack_ancestors turns them back into the int64 / int32 arrays for everything else.

The int64 path is the reference everywhere — the entries that take the two arrays, or `settings.packed_ancestors` off —
and every comparison is for equal bits: the packed forms change what is loaded and stored, not what is computed.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_linear_gaussian import operands
from tests.test_gpu_noise_and_lazy_latents import _ancestors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kernels(hip_device):
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def seed(value):
    torch.manual_seed(value)
    np.random.seed(value)


# ---- K2 -------------------------------------------------------------------------------------------------------------
def _rows(K, dtype, device):
    """B = 5 rows: N(0,1); collapsed (one weight 40 above the rest); exact-zero weights (-inf entries); all -inf; a NaN."""
    gen = torch.Generator().manual_seed(K)
    lw = torch.randn(5, K, generator=gen, dtype=torch.float64)
    lw[1, K // 3] += 40.0
    lw[2, torch.rand(K, generator=gen) < 0.4] = float("-inf")
    lw[3] = float("-inf")
    lw[4, K // 2] = float("nan")
    return lw.to(dtype).to(device)


def _raw_step(kernels, lw, u, ranges, packed):
    """One raw launch: (idx int64, child_end int32 or None, lse, flags) — the packed entry's words taken apart on the host
    side of the comparison with integer arithmetic (not with the unpack launch: that has a test of its own)."""
    from aesmc_amd._kernels import _DTYPE_TAG, _ptr
    lib, dev = kernels._lib, lw.device
    B, K = lw.shape
    kernels.read_flags(dev)
    lse = torch.full((B,), 7.0, dtype=lw.dtype, device=dev)
    if packed:
        words = torch.full((B, K), -1, dtype=torch.int32, device=dev)
        status = lib.aesmc_resample_step_packed(_DTYPE_TAG[lw.dtype], _ptr(lw), _ptr(u), _ptr(words), _ptr(lse), 1 if ranges else 0,
                                                _ptr(kernels.flags(dev)), B, K, kernels._stream(lw))
        assert status == 0
        wide = words.to(torch.int64) & 0xffffffff
        idx, ends = wide & 0xffff, (wide >> 16).to(torch.int32)
    else:
        idx = torch.full((B, K), -1, dtype=torch.int64, device=dev)
        ends = torch.full((B, K), -1, dtype=torch.int32, device=dev) if ranges else None
        if ranges:
            status = lib.aesmc_resample_step_ranges(_DTYPE_TAG[lw.dtype], _ptr(lw), _ptr(u), _ptr(idx), _ptr(lse), _ptr(ends),
                                                    _ptr(kernels.flags(dev)), B, K, kernels._stream(lw))
        else:
            status = lib.aesmc_resample_step(_DTYPE_TAG[lw.dtype], _ptr(lw), _ptr(u), _ptr(idx), _ptr(lse), None, None,
                                             _ptr(kernels.flags(dev)), B, K, 0, 0, 0, kernels._stream(lw))
        assert status == 0
    return idx, ends, lse, kernels.read_flags(dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("K", [768, 1024, 4096, 8192])
def test_packed_resampling_step_equals_the_two_arrays(kernels, hip_device, dtype, K):
    """word & 0xffff == idx and word >> 16 == child_end for every particle, the row log-sum-exp and the flags identical;
    without the ranges the high halves are 0.  K = 768 .. 4096: four particles per lane, 8192: eight — the rows for which
    the int64 entries run the lean kernel themselves (asserted), by their own dispatch: the comparison is of the library
    with the hand-off against the library without it.  u = 0 and u just below 1 on rows 0 and 2."""
    from aesmc_amd import _lib
    lib = kernels._lib
    lw = _rows(K, dtype, hip_device)
    u = torch.tensor([0.0, 0.37, 1.0 - 2.0 ** -53, 0.5, 0.5], dtype=torch.float64, device=hip_device)
    want = _raw_step(kernels, lw, u, True, False)
    assert lib.aesmc_test_last_k2_form() == 2
    got = _raw_step(kernels, lw, u, True, True)
    plain_want = _raw_step(kernels, lw, u, False, False)
    plain_got = _raw_step(kernels, lw, u, False, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2].cpu().numpy().tobytes() == want[2].cpu().numpy().tobytes()      # (bits: the NaN row's lse is NaN)
    assert got[3] == want[3] == (_lib.FLAG_DEGENERATE_ROW | _lib.FLAG_NAN_LOG_WEIGHT)
    assert bool((got[0][3:] == K).all()) and int(got[1][3:].abs().max()) == 0      # degenerate and NaN rows: K, no children
    assert int(got[1][:2, -1].min()) == K == int(got[1][:2, -1].max())
    assert torch.equal(plain_got[0], plain_want[0]) and torch.equal(plain_got[0], want[0])
    assert int(plain_got[1].abs().max()) == 0
    assert plain_got[2].cpu().numpy().tobytes() == plain_want[2].cpu().numpy().tobytes() and plain_got[3] == plain_want[3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rows_of_256_particles_are_declined_and_take_the_two_arrays(kernels, hip_device, dtype):
    """K = 256 (and every row of at most 512 particles): the int64 step runs the general kernel at two particles per lane
    there, which has no packed form — the packed entry declines (AESMC_ERR_UNSUPPORTED, nothing launched, nothing
    written) and the provider hands out the int64 indices and int32 ranges of the step it has always run, bit for bit."""
    from aesmc_amd import _lib
    from aesmc_amd._kernels import _DTYPE_TAG, _ptr
    K = 256
    lw = _rows(K, dtype, hip_device)
    u = torch.tensor([0.0, 0.37, 1.0 - 2.0 ** -53, 0.5, 0.5], dtype=torch.float64, device=hip_device)
    kernels.read_flags(hip_device)
    words = torch.full((5, K), -1, dtype=torch.int32, device=hip_device)
    lse = torch.full((5,), 7.0, dtype=dtype, device=hip_device)
    for ranges in (0, 1):
        status = kernels._lib.aesmc_resample_step_packed(_DTYPE_TAG[dtype], _ptr(lw), _ptr(u), _ptr(words), _ptr(lse), ranges,
                                                         _ptr(kernels.flags(hip_device)), 5, K, kernels._stream(lw))
        assert status == _lib.ERR_UNSUPPORTED
    assert bool((words == -1).all()) and bool((lse == 7.0).all()) and kernels.read_flags(hip_device) == 0
    want = _raw_step(kernels, lw, u, True, False)
    idx, got_lse, _ = kernels.resample_step(lw, u, None, want_lse=True, want_child_end=True, packed=True)
    flags = kernels.read_flags(hip_device)
    assert torch.is_tensor(idx) and idx.dtype == torch.int64 and torch.equal(idx, want[0])
    assert torch.equal(idx._aesmc_child_end, want[1]) and flags == want[3]
    assert got_lse.cpu().numpy().tobytes() == want[2].cpu().numpy().tobytes()


def test_unpack_gives_the_two_arrays_once(kernels, hip_device):
    """`PackedAncestors.index()` / `.child_end()`: one launch, memoised, int64 / int32, what the ranges entry wrote."""
    from aesmc_amd._kernels import PackedAncestors
    kernels.read_flags(hip_device)
    gen = torch.Generator().manual_seed(3)
    lw = torch.randn(5, 1024, generator=gen, dtype=torch.float64).float().to(hip_device)
    u = torch.rand(5, generator=gen, dtype=torch.float64).to(hip_device)
    idx, lse, _ = kernels.resample_step(lw, u, None, want_lse=True, want_child_end=True)
    handle, lse_packed, moved = kernels.resample_step(lw, u, None, want_lse=True, want_child_end=True, packed=True)
    assert type(handle) is PackedAncestors and handle.has_ranges and moved is None and handle.words.dtype == torch.int32
    assert torch.equal(lse, lse_packed)
    unpacked = handle.index()
    assert unpacked.dtype == torch.int64 and torch.equal(unpacked, idx) and unpacked._aesmc_sorted is True
    assert handle.child_end().dtype == torch.int32 and torch.equal(handle.child_end(), idx._aesmc_child_end)
    assert handle.index() is unpacked
    bare, _, _ = kernels.resample_step(lw, u, None, packed=True)
    assert type(bare) is PackedAncestors and bare.child_end() is None and torch.equal(bare.index(), idx)
    # the three conveniences of a wrapper that records or overrides a step's ancestors; `copy_` reaches the words
    assert not torch.is_tensor(handle) and not hasattr(handle, "dtype")      # (no tensor face: nothing unpacks by accident)
    assert handle.clone().dtype == torch.int64 and torch.equal(handle.clone(), idx) and torch.equal(handle.cpu(), idx.cpu())
    other = kernels.resample_step(lw.flip(1), u, None, want_child_end=True)[0]
    assert not torch.equal(other, idx)
    handle.copy_(other)
    again = PackedAncestors(handle.words.clone(), True)
    assert torch.equal(again.index(), other) and torch.equal(again.child_end(), other._aesmc_child_end)
    assert kernels.read_flags(hip_device) == 0


# ---- K16 ------------------------------------------------------------------------------------------------------------
def _drawn(kernels, x_prev, ancestors, y, terms, scales, paired, packed):
    """One raw launch of K16 through the int64 indices or the packed words: (x_t, lw, flags)."""
    from aesmc_amd import _philox
    from aesmc_amd._kernels import _ptr
    dev = x_prev.device
    B, K, dx = x_prev.shape
    kernels.read_flags(dev)
    maps = [kernels._affine_map(*term) for term in terms]
    pairs = kernels._build_pairs(maps, list(scales), dev) if paired else None
    torch.manual_seed(5)
    reservation = _philox.reserve(B * K * dx, dev)
    out_x = torch.full_like(x_prev, float("nan"))
    lw = torch.full((B, K), float("nan"), device=dev)
    entry = kernels._lib.aesmc_affine_normal_propagate_drawn_packed if packed else \
        kernels._lib.aesmc_affine_normal_propagate_drawn_paired
    status = entry(_ptr(x_prev), _ptr(ancestors), _ptr(y), y.stride(0), ctypes.byref(maps[0][0]), ctypes.byref(maps[1][0]),
                   ctypes.byref(maps[2][0]), _ptr(scales[0]), _ptr(scales[1]), _ptr(scales[2]), _ptr(out_x), _ptr(lw),
                   _ptr(kernels.flags(dev)), B, K, reservation.seed, reservation.offset, reservation.threads,
                   _ptr(reservation.state), _ptr(pairs), kernels._stream(x_prev))
    assert status == 0
    return out_x, lw, kernels.read_flags(dev)


def _words_of(idx, high):
    """int32 [B,K] holding idx | high << 16 as uint32 bits."""
    wide = idx | (high.to(torch.int64) << 16)
    return torch.where(wide >= 2 ** 31, wide - 2 ** 32, wide).to(torch.int32)


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("dy_is_dx", [True, False])
@pytest.mark.parametrize("d", [3, 10, 16])
@pytest.mark.parametrize("B,K", [(5, 512), (3, 4096)])
def test_k16_through_packed_words_equals_k16_through_int64(kernels, hip_device, B, K, d, dy_is_dx, paired):
    """x_t and the log-weights bit for bit, the same seed and offset on both routes; the high halves (the ranges of a real
    step, all sixteen bits used) do not reach the result.  A row whose low halves are K raises the flag the int64 launch
    raises for the index K, reads the row K - 1 as it does, and does not fault."""
    from aesmc_amd import _lib
    dy = d if dy_is_dx else 1
    _, o = operands(B, K, d, dy, np.float32, hip_device, seed=B + K + d)
    idx = _ancestors(B, K, hip_device, seed=B + K, spread=1.0)
    gen = torch.Generator().manual_seed(d)
    high = torch.randint(0, 65536, (B, K), generator=gen).to(hip_device)
    terms = ((o["A"], None), (o["C"], o["off_g"]), (o["Q"], o["off_q"]))
    scales = (o["s_p"], o["s_g"], o["s_q"])
    want = _drawn(kernels, o["x_prev"], idx, o["y"], terms, scales, paired, False)
    got = _drawn(kernels, o["x_prev"], _words_of(idx, high), o["y"], terms, scales, paired, True)
    assert kernels._lib.aesmc_test_last_k16_form() == 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2] == 0
    bad = idx.clone()
    bad[B - 1] = K
    want = _drawn(kernels, o["x_prev"], bad, o["y"], terms, scales, paired, False)
    got = _drawn(kernels, o["x_prev"], _words_of(bad, torch.zeros_like(high)), o["y"], terms, scales, paired, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2] == want[2] == _lib.FLAG_INDEX_OUT_OF_RANGE


# ---- K14 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [10, 4])
def test_k14_through_packed_words_equals_k14_through_the_two_arrays(kernels, hip_device, d):
    """B = 4, K = 512: the step's ancestors out of one resampling's words, the parent's gradient arriving through the
    children ranges of the NEXT resampling's words (healthy and collapsed: runs a lane sums alone, runs the wavefront
    shares out) — every gradient bit-equal to the launch that reads the int64 indices and the int32 ranges; also with
    only one of the two (the run's last step has no children, and a mix of a handle and a tensor is unpacked).  (Rows of
    512 particles: the int64 resampling step's own arrays, packed into words here — the packed step serves longer rows.)"""
    from aesmc_amd._kernels import PackedAncestors
    B, K = 4, 512
    _, o = operands(B, K, d, d, np.float32, hip_device, seed=3 * B + K + d)
    off_p = torch.from_numpy(np.random.RandomState(4).randn(d).astype(np.float32)).to(hip_device)
    terms = ((o["A"], off_p), (o["C"], o["off_g"]), (o["Q"], o["off_q"]))
    scales = (o["s_p"], o["s_g"], o["s_q"])
    need = [True] * 12
    need[1] = False

    def resampling(seed_, spread):
        gen = torch.Generator().manual_seed(seed_)
        lw = (spread * torch.randn(B, K, generator=gen, dtype=torch.float64)).float().to(hip_device)
        u = torch.rand(B, generator=gen, dtype=torch.float64).to(hip_device)
        idx = kernels.resample_step(lw, u, None, want_child_end=True)[0]
        ends = idx._aesmc_child_end
        return PackedAncestors(_words_of(idx, ends), True), idx, ends

    here, idx, _ = resampling(1, 2.0)
    moved = kernels.gather(o["x_prev"], idx)
    x = kernels.affine_rsample(moved, o["Q"], o["off_q"], o["eps"], o["s_q"])
    lw = kernels.affine_logweight(moved, x, o["y"], *terms, scales)
    _, lse = kernels.logweight_lse(lw, None, None, want_lw=False)
    rng = np.random.RandomState(9)
    grad_lse = torch.from_numpy(rng.randn(B).astype(np.float32)).to(hip_device)
    child_grad = torch.from_numpy(rng.randn(B, K, d).astype(np.float32)).to(hip_device)
    lib = kernels._lib
    for spread in (1.0, 9.0):
        after, _, ends = resampling(2, spread)
        assert spread < 5 or int((ends[:, 1:] - ends[:, :-1]).max()) > 32
        want = kernels.affine_step_backward(o["x_prev"], x, o["y"], *terms, scales, need, lw, lse, grad_lse=grad_lse,
                                            ancestors=idx, child_grad=child_grad, child_end=ends)
        assert lib.aesmc_test_last_step_backward_form() == 2
        calls = {"packed": 0}
        real = lib.aesmc_affine_step_backward_packed

        def counting(*args):
            calls["packed"] += 1
            return real(*args)
        counting.__name__ = real.__name__
        lib.aesmc_affine_step_backward_packed = counting
        try:
            got = kernels.affine_step_backward(o["x_prev"], x, o["y"], *terms, scales, need, lw, lse, grad_lse=grad_lse,
                                               ancestors=here, child_grad=child_grad, child_end=after)
            assert calls["packed"] == 1
            mixed = kernels.affine_step_backward(o["x_prev"], x, o["y"], *terms, scales, need, lw, lse, grad_lse=grad_lse,
                                                 ancestors=here, child_grad=child_grad, child_end=ends)
            assert calls["packed"] == 1
        finally:
            lib.aesmc_affine_step_backward_packed = real
        for a, b, c in zip(got, want, mixed):
            assert (a is None and b is None) or (torch.equal(a, b) and torch.equal(c, b))
    want = kernels.affine_step_backward(o["x_prev"], x, o["y"], *terms, scales, need, lw, lse, grad_lse=grad_lse, ancestors=idx)
    got = kernels.affine_step_backward(o["x_prev"], x, o["y"], *terms, scales, need, lw, lse, grad_lse=grad_lse, ancestors=here)
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)
    assert kernels.read_flags(hip_device) == 0


# ---- end to end -----------------------------------------------------------------------------------------------------
def _model(hip_device, d, B, T):
    from aesmc_amd.testing import models
    model = models.LgssmNd(d, seed=0, validate_args=False, affine=True).to(hip_device)
    observations = model.simulate(T, B, seed=1)
    return model, observations, (model.initial, model.transition, model.emission, model.proposal)


def _count_packed_steps(kernels):
    """Wraps the library's packed resampling entry and its unpack entry: how many launches went through each."""
    lib = kernels._lib
    real, real_unpack = lib.aesmc_resample_step_packed, lib.aesmc_unpack_ancestors
    calls = {"n": 0, "unpack": 0}

    def counting(*args):
        calls["n"] += 1
        return real(*args)

    def counting_unpack(*args):
        calls["unpack"] += 1
        return real_unpack(*args)
    counting.__name__, counting_unpack.__name__ = real.__name__, real_unpack.__name__
    lib.aesmc_resample_step_packed, lib.aesmc_unpack_ancestors = counting, counting_unpack

    def restore():
        lib.aesmc_resample_step_packed, lib.aesmc_unpack_ancestors = real, real_unpack
    return calls, restore


@pytest.mark.parametrize("d,B,K,T", [(3, 8, 256, 5), (10, 4, 512, 4), (4, 8, 768, 5), (10, 4, 1024, 4)])
def test_loss_and_gradients_are_the_same_bits_with_the_switch_on_and_off(kernels, hip_device, d, B, K, T):
    """get_loss(..., 'aesmc'): the loss and every parameter gradient, eager and through GraphedLoss.  Rows of 256 and 512
    particles: the switch selects nothing there (the step runs the general kernel, which has no packed form); 768 and
    1024 (rows of an even number of values, which K14's rows form takes): every resampling step of the run goes through the packed entry, the forward pass unpacks NOTHING and the
    backward pass exactly once (the run's first step sums its children through the int32 ranges)."""
    from aesmc_amd import graphs, losses, settings
    model, observations, parts = _model(hip_device, d, B, T)
    results = {}
    for packed in (False, True):
        calls, restore = _count_packed_steps(kernels)
        try:
            with settings.override(packed_ancestors=packed):
                seed(11)
                loss = losses.get_loss(observations, K, "aesmc", *parts)
                in_effect = packed and K > 512
                assert calls["n"] == (T - 1 if in_effect else 0), "the switch does not select the route"
                assert calls["unpack"] == 0, "the forward pass unpacked a step's words"
                loss.backward()
                assert calls["unpack"] == (1 if in_effect else 0), "the backward pass unpacks once per run"
                eager = (loss.detach().clone(), [p.grad.clone() for p in model.parameters()])
                del loss
                model.zero_grad(set_to_none=True)
                graphed = graphs.GraphedLoss(observations, K, "aesmc", *parts, backward=True)
                seed(11)
                replayed = (graphed().detach().clone(), [p.grad.clone() for p in model.parameters()])
                del graphed
                model.zero_grad(set_to_none=True)
        finally:
            restore()
        results[packed] = (eager, replayed)
    for route in (0, 1):
        (loss_off, grads_off), (loss_on, grads_on) = results[False][route], results[True][route]
        assert torch.equal(loss_on, loss_off)
        assert len(grads_on) == len(grads_off) > 0
        for a, b in zip(grads_on, grads_off):
            assert torch.equal(a, b)


def test_what_infer_returns_is_int64_and_equal(kernels, hip_device):
    from aesmc_amd import inference, settings
    model, observations, parts = _model(hip_device, 3, 8, 5)
    out = {}
    for packed in (False, True):
        calls, restore = _count_packed_steps(kernels)
        try:
            with settings.override(packed_ancestors=packed), torch.no_grad():
                seed(4)
                out[packed] = inference.infer("smc", observations, *parts, 1024, return_log_marginal_likelihood=True,
                                              return_ancestral_indices=True, return_latents=True)
        finally:
            restore()
        assert calls["n"] == (4 if packed else 0)
    for a, b in zip(out[True]["ancestral_indices"], out[False]["ancestral_indices"]):
        assert a.dtype == torch.int64 and torch.is_tensor(a) and torch.equal(a, b)
    for a, b in zip(out[True]["latents"], out[False]["latents"]):
        assert torch.equal(a, b)
    assert torch.equal(out[True]["log_marginal_likelihood"], out[False]["log_marginal_likelihood"])


def test_a_model_that_reads_the_resampled_values_mid_run(kernels, hip_device):
    """The proposal of timestep 2 reads previous_latents[-1] as numbers (PyTorch arithmetic on it): the handle unpacks
    for the gather, and the run equals the one with the switch off."""
    from aesmc_amd import inference, settings
    model, observations, parts = _model(hip_device, 3, 8, 5)
    initial, transition, emission, proposal = parts
    read = []

    def reading(previous_latents=None, time=None, observations=None):
        if time == 2:
            read.append(float(previous_latents[-1].abs().sum()))
        return proposal(previous_latents=previous_latents, time=time, observations=observations)

    out = {}
    for packed in (False, True):
        with settings.override(packed_ancestors=packed), torch.no_grad():
            seed(6)
            out[packed] = inference.infer("smc", observations, initial, transition, emission, reading, 1024,
                                          return_log_marginal_likelihood=True, return_latents=False)
    assert len(read) == 2 and read[0] == read[1]
    assert torch.equal(out[True]["log_marginal_likelihood"], out[False]["log_marginal_likelihood"])
    assert torch.equal(out[True]["last_latent"], out[False]["last_latent"])


def test_seventy_thousand_particles_take_the_old_path(kernels, hip_device):
    """K = 70000 does not fit sixteen bits (nor one workgroup): the step runs as before, whatever the switch says."""
    from aesmc_amd import inference, settings
    model, observations, parts = _model(hip_device, 3, 1, 3)
    calls, restore = _count_packed_steps(kernels)
    try:
        with settings.override(packed_ancestors=True), torch.no_grad():
            seed(8)
            out = inference.infer("smc", observations, *parts, 70000, return_log_marginal_likelihood=True,
                                  return_ancestral_indices=True, return_latents=False)
    finally:
        restore()
    assert calls["n"] == 0
    assert all(index.dtype == torch.int64 and 0 <= int(index.min()) and int(index.max()) < 70000
               for index in out["ancestral_indices"])
    assert torch.isfinite(out["log_marginal_likelihood"]).all()
