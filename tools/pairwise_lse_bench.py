"""The pairwise log-sum-exp launch (aesmc_pairwise_lse, K22: half of one backward step of the marginal smoother) beside
the PyTorch float64 composition of the same contract on the same device — a broadcast difference, sum and logsumexp,
chunked over the row points so that its [B, r, C, D] float64 intermediate fits in memory — and beside the kernel's other
forms (tile height 8 / 16, one / four wavefronts per workgroup, one pass / K21's two), walked through the test hook.
Everything is timed warm between HIP events, one launch (one composition) per pair of events, the forms alternating
within each repetition; the median is reported with the spread.  Operations are the ALGORITHM's (one score and one
exponential per pair, whatever a form spends), so the share of the float64 vector peak compares the forms directly.
    python tools/pairwise_lse_bench.py [B,R,C,D ...]        (default: 1024,4096,4096,10 and 64,1024,1024,10; float32)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
PEAK_FP64_VECTOR = 78.6e12      # MI355X, float64 vector FLOP/s (a fused multiply-add counts two)
EXP_FLOPS = 34                  # exp_nonpositive: rint, a product, two + thirteen fused multiply-adds, ldexp
FORMS = [(8, 4, 1), (16, 4, 1), (8, 1, 1), (16, 1, 1), (8, 4, 2), (16, 4, 2), (8, 1, 2), (16, 1, 2)]


def composition(rows, cols, scale, col_a, col_sub, row_add, chunk):
    B, R = row_add.shape
    term, c, inv = (col_a.double() - col_sub.double())[:, None, :], cols.double()[:, None, :, :], 1.0 / scale.double()
    out = torch.empty(B, R, dtype=torch.float64, device=rows.device)
    for r0 in range(0, R, chunk):
        diff = (rows[:, r0:r0 + chunk].double()[:, :, None, :] - c) * inv
        out[:, r0:r0 + chunk] = torch.logsumexp(term - 0.5 * (diff * diff).sum(-1), dim=-1)
    return (row_add.double() + out).to(row_add.dtype)


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


def form(tile, waves, passes):
    def launch():
        assert k._lib.aesmc_test_set_pairwise_lse_form(tile, waves, passes) == 0
        return k.pairwise_lse(*operands)
    return launch


print("tools/pairwise_lse_bench.py on one {} ({}), float32 operands, HIP events, warm".format(
    torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode()))
for spec in sys.argv[1:] or ["1024,4096,4096,10", "64,1024,1024,10"]:
    B, R, C, D = [int(v) for v in spec.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
    rows, cols, col_a, col_sub, row_add = rand(B, R, D), rand(B, C, D), rand(B, C), rand(B, C), rand(B, R)
    scale = torch.full((1,), 0.9, device=dev)
    operands = (rows, cols, scale, col_a, col_sub, row_add)
    chunk = max(1, min(R, (1 << 31) // (B * C * D * 8)))      # 2 GiB for the [B, chunk, C, D] float64 difference
    pairs = B * R * C
    flops = pairs * (4 * D + 5 + EXP_FLOPS)      # (sub, mul, fma) per d, the score, s - ref, one exp, the sum, the vote
    print("B={} R={} C={} D={} float32: {:.3e} pairs, {:.3e} float64 operations; us, median (min .. max)".format(
        B, R, C, D, pairs, flops))
    try:
        theirs = composition(*operands, chunk)
        differences = []
        for tile, waves, passes in FORMS:
            differences.append(float((form(tile, waves, passes)().double() - theirs.double()).abs().max()))
        reps = 5 if pairs > 1e10 else 21
        results = timed([form(*f) for f in FORMS], 2, reps)
        assert k._lib.aesmc_test_set_pairwise_lse_form(0, 0, 0) == 0
        default = timed([lambda: k.pairwise_lse(*operands)], 2, reps)[0]
        torch_ = timed([lambda: composition(*operands, chunk)], 1, 3)[0]
    finally:
        k._lib.aesmc_test_set_pairwise_lse_form(0, 0, 0)
    share = lambda t: (flops / t / 1e6, 100 * flops / t / 1e-6 / PEAK_FP64_VECTOR)
    for (tile, waves, passes), result, difference in zip(FORMS, results, differences):
        print("  kernel K22, {:2d} row points x {} wavefront{}, {} pass{:2s} {:10.1f} ({:.1f} .. {:.1f})   {:5.2f} TFLOP/s = {:4.1f} % "
              "of the float64 vector peak; largest difference from the composition {:.1e}".format(
                  tile, waves, " " if waves == 1 else "s", passes, "" if passes == 1 else "es", *result, *share(result[0]),
                  difference))
    print("  kernel K22 as the library launches it        {:10.1f} ({:.1f} .. {:.1f})   {:5.2f} TFLOP/s = {:4.1f} % of the "
          "float64 vector peak (compute-bound: {:.1f} MB of operands)".format(
              *default, *share(default[0]), 4e-6 * B * ((R + C) * D + 2 * (R + C))))
    print("  PyTorch float64 composition                  {:10.1f} ({:.1f} .. {:.1f})   {} row points per chunk".format(
        *torch_, chunk))
    print("  composition / kernel at the medians: {:.1f}x".format(torch_[0] / default[0]), flush=True)
