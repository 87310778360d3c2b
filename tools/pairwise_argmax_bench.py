"""The pairwise max-and-argmax launch (aesmc_pairwise_argmax, K24: one step of the MAP trajectory's Viterbi recursion)
beside K22 (aesmc_pairwise_lse) on the SAME operands in the same run — K24 does K22's score work without the
exponentials, so K22's time is the yardstick — and beside the PyTorch float64 composition of the same contract on the same
device: a broadcast difference, a sum and a max with its index, chunked over the row points so that its [B, r, C, D]
float64 intermediate fits in memory.  Everything is timed warm between HIP events, one launch (one composition) per
pair of events, the two kernels alternating within each repetition; the median is reported with the spread.  Operations
are the ALGORITHM's (one score, one comparison and one select per pair).
    python tools/pairwise_argmax_bench.py [B,R,C,D ...]      (default: 1024,4096,4096,10 and 64,1024,1024,10; float32)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
PEAK_FP64_VECTOR = 78.6e12      # MI355X, float64 vector FLOP/s (a fused multiply-add counts two)


def composition(rows, cols, scale, col_a, col_sub, row_add, chunk):
    B, R = row_add.shape
    term, c, inv = (col_a.double() - col_sub.double())[:, None, :], cols.double()[:, None, :, :], 1.0 / scale.double()
    out = torch.empty(B, R, dtype=torch.float64, device=rows.device)
    arg = torch.empty(B, R, dtype=torch.int64, device=rows.device)
    for r0 in range(0, R, chunk):
        diff = (rows[:, r0:r0 + chunk].double()[:, :, None, :] - c) * inv
        out[:, r0:r0 + chunk], arg[:, r0:r0 + chunk] = torch.max(term - 0.5 * (diff * diff).sum(-1), dim=-1)
    return (row_add.double() + out).to(row_add.dtype), arg


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


print("tools/pairwise_argmax_bench.py on one {} ({}), float32 operands, HIP events, warm".format(
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
    flops = pairs * (4 * D + 4)      # (sub, mul, fma) per d, the score's fused multiply-add, one comparison, one select
    print("B={} R={} C={} D={} float32: {:.3e} pairs, {:.3e} float64 operations; us, median (min .. max)".format(
        B, R, C, D, pairs, flops))
    theirs, their_arg = composition(*operands, chunk)
    mine, my_arg = k.pairwise_argmax(*operands)
    difference = float((mine.double() - theirs.double()).abs().max())
    same = float((my_arg == their_arg).double().mean())
    assert k.read_flags(dev) == 0
    reps = 5 if pairs > 1e10 else 21
    argmax, lse = timed([lambda: k.pairwise_argmax(*operands), lambda: k.pairwise_lse(*operands)], 2, reps)
    torch_ = timed([lambda: composition(*operands, chunk)], 1, 3)[0]
    print("  kernel K24 (pairwise_argmax)                 {:10.1f} ({:.1f} .. {:.1f})   {:5.2f} TFLOP/s = {:4.1f} % of the float64 "
          "vector peak (compute-bound: {:.1f} MB of operands); largest difference from the composition {:.1e}, the same "
          "column at {:.4f} % of the row points".format(
              *argmax, flops / argmax[0] / 1e6, 100 * flops / argmax[0] / 1e-6 / PEAK_FP64_VECTOR,
              4e-6 * B * ((R + C) * D + 2 * (R + C)) + 8e-6 * B * R, difference, 100 * same))
    print("  kernel K22 (pairwise_lse), the same operands {:10.1f} ({:.1f} .. {:.1f})".format(*lse))
    print("  PyTorch float64 composition                  {:10.1f} ({:.1f} .. {:.1f})   {} row points per chunk".format(
        *torch_, chunk))
    print("  K24 / K22 at the medians: {:.2f}x; composition / K24: {:.1f}x".format(argmax[0] / lse[0], torch_[0] / argmax[0]),
          flush=True)
