"""The pairwise softmax-mean launch (aesmc_pairwise_mean, K23: the first half of one backward step of the two-slice
smoother) in every form — the float64 matrix cores, the vector pipe with 4 x 16 and 2 x 32 accumulators per lane, walked
through the test hook — beside the PyTorch float64 composition of the same contract on the same device (a broadcast
difference, a softmax and a batched product, chunked over the row points so that its [B, r, C, D] float64 intermediate fits
in memory) and beside K22 (aesmc_pairwise_lse, the launch K23 replaces) on the same operands.  Everything is timed warm
between HIP events, one launch (one composition) per pair of events, the kernels alternating within each repetition; the
median is reported with the spread.
    python tools/pairwise_mean_bench.py [--k22-library PATH] [B,R,C,D,P ...]
        (default: 64,1024,1024,10,10 and 64,1024,1024,10,64; float32)
--k22-library: another build of the library (the parent commit's) whose aesmc_pairwise_lse is timed in the same run."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels, _lib  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
FORMS = [(1, "matrix cores, 16 row points"), (2, "vector pipe, 4 row points x 16"), (3, "vector pipe, 2 row points x 32")]


def composition(rows, cols, scale, col_a, payload, chunk):
    B, R = rows.shape[:2]
    term, c, inv = col_a.double()[:, None, :], cols.double()[:, None, :, :], 1.0 / scale.double()
    pay = payload.double()
    out = torch.empty(B, R, payload.shape[2], dtype=torch.float64, device=rows.device)
    lse = torch.empty(B, R, dtype=torch.float64, device=rows.device)
    for r0 in range(0, R, chunk):
        diff = (rows[:, r0:r0 + chunk].double()[:, :, None, :] - c) * inv
        s = term - 0.5 * (diff * diff).sum(-1)
        lse[:, r0:r0 + chunk] = torch.logsumexp(s, dim=-1)
        out[:, r0:r0 + chunk] = torch.bmm(torch.softmax(s, dim=-1), pay)
    return out.to(rows.dtype), lse.to(rows.dtype)


def timed(fns, warm, reps):
    """Median, min and max in microseconds of every callable of `fns`, taken in turn within each repetition."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, record in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            record.append(a.elapsed_time(b) * 1e3)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def form(number):
    def launch():
        assert k._lib.aesmc_test_set_pairwise_mean_form(number) == 0
        return k.pairwise_mean(*operands)
    return launch


def other_k22(path, rows, cols, scale, col_a):
    """aesmc_pairwise_lse of the library at `path` on the same operands (dense, one scale value)."""
    lib = ctypes.CDLL(path)
    entry = lib.aesmc_pairwise_lse
    entry.restype, entry.argtypes = _lib.SIGNATURES["aesmc_pairwise_lse"]
    B, R, D = rows.shape
    out = torch.empty(B, R, dtype=rows.dtype, device=rows.device)
    views = [_lib.View3(t.data_ptr(), *t.stride()) for t in (rows, cols)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        status = entry(0, ctypes.byref(views[0]), ctypes.byref(views[1]), scale.data_ptr(), 0, col_a.data_ptr(), None, None,
                       out.data_ptr(), k.flags(dev).data_ptr(), B, R, cols.shape[1], D, stream)
        assert status == 0
        return out
    return launch


arguments = sys.argv[1:]
k22_library = None
if arguments[:1] == ["--k22-library"]:
    k22_library, arguments = arguments[1], arguments[2:]
print("tools/pairwise_mean_bench.py on one {} ({}), float32 operands, HIP events, warm".format(
    torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode()))
for spec in arguments or ["64,1024,1024,10,10", "64,1024,1024,10,64"]:
    B, R, C, D, P = [int(v) for v in spec.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
    rows, cols, col_a, payload = rand(B, R, D), rand(B, C, D), rand(B, C), rand(B, C, P)
    scale = torch.full((1,), 0.9, device=dev)
    operands = (rows, cols, scale, col_a, payload)
    chunk = max(1, min(R, (1 << 31) // (B * C * D * 8)))      # 2 GiB for the [B, chunk, C, D] float64 difference
    pairs = B * R * C
    print("B={} R={} C={} D={} P={} float32: {:.3e} pairs, {:.3e} payload multiply-adds; us, median (min .. max)".format(
        B, R, C, D, P, pairs, pairs * P))
    try:
        theirs, their_lse = composition(*operands, chunk)
        differences = []
        for number, _ in FORMS:
            mine, my_lse = form(number)()
            differences.append((float((mine.double() - theirs.double()).abs().max()),
                                float((my_lse.double() - their_lse.double()).abs().max())))
        results = timed([form(number) for number, _ in FORMS], 2, 21)
        assert k._lib.aesmc_test_set_pairwise_mean_form(0) == 0
        kernels = [lambda: k.pairwise_mean(*operands), lambda: k.pairwise_lse(rows, cols, scale, col_a)]
        if k22_library is not None:
            kernels.append(other_k22(k22_library, rows, cols, scale, col_a))
            assert torch.equal(kernels[2](), kernels[1]())          # K22's bits are what they were
        default, k22, *parent = timed(kernels, 2, 21)
        torch_ = timed([lambda: composition(*operands, chunk)], 1, 3)[0]
    finally:
        k._lib.aesmc_test_set_pairwise_mean_form(0)
    for (number, name), result, difference in zip(FORMS, results, differences):
        print("  kernel K23, form {} ({:31s}) {:10.1f} ({:.1f} .. {:.1f})   largest difference from the composition {:.1e} "
              "(lse {:.1e})".format(number, name, *result, *difference))
    print("  kernel K23 as the library launches it             {:10.1f} ({:.1f} .. {:.1f})".format(*default))
    print("  kernel K22 on the same operands, this library     {:10.1f} ({:.1f} .. {:.1f})".format(*k22))
    reference = k22
    if parent:
        reference = parent[0]
        print("  kernel K22 on the same operands, --k22-library    {:10.1f} ({:.1f} .. {:.1f})   the same bits".format(*reference))
    print("  PyTorch float64 composition                       {:10.1f} ({:.1f} .. {:.1f})   {} row points per chunk".format(
        *torch_, chunk))
    print("  K23 / K22 at the medians: {:.2f}x      composition / K23 at the medians: {:.1f}x".format(
        default[0] / reference[0], torch_[0] / default[0]), flush=True)
