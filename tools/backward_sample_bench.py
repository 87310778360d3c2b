"""The backward-simulation launch (aesmc_backward_sample, K21) beside the PyTorch float64 composition of the same contract
on the same device — a broadcast difference, sum, exp, cumsum and searchsorted, chunked over the trajectories so that
its [B, m, K, D] float64 intermediate fits in memory.  Both are timed warm between HIP events, one launch (one
composition) per pair of events, and the median is reported with the spread.
    python tools/backward_sample_bench.py [B,K,M,D ...]        (default: 1024,4096,128,10 and 64,1024,1024,10; float32)"""
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


def composition(log_w, loc, target, scale, u, rows):
    B, K = log_w.shape
    M = u.size(1)
    lw, l, inv = log_w.double(), loc.double(), 1.0 / scale.double()
    idx = torch.empty(B, M, dtype=torch.int64, device=log_w.device)
    for m0 in range(0, M, rows):
        t = target[:, m0:m0 + rows].double()
        diff = (t[:, :, None, :] - l[:, None, :, :]) * inv
        s = lw[:, None, :] - 0.5 * (diff * diff).sum(-1)
        c = torch.exp(s - s.max(-1, keepdim=True).values).cumsum(-1)
        thr = u[:, m0:m0 + rows] * c[..., -1]
        idx[:, m0:m0 + rows] = torch.searchsorted(c, thr.unsqueeze(-1), right=True).squeeze(-1).clamp_(max=K - 1)
    return idx


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


for spec in sys.argv[1:] or ["1024,4096,128,10", "64,1024,1024,10"]:
    B, K, M, D = [int(v) for v in spec.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    log_w = torch.randn(B, K, device=dev, generator=gen)
    loc = torch.randn(B, K, D, device=dev, generator=gen)
    target = torch.randn(B, M, D, device=dev, generator=gen)
    scale = torch.full((1,), 0.9, device=dev)
    u = torch.rand(B, M, device=dev, dtype=torch.float64, generator=gen)
    rows = max(1, min(M, (1 << 31) // (B * K * D * 8)))      # 2 GiB for the [B, rows, K, D] float64 difference
    mine = k.backward_sample(log_w, loc, target, scale, u)[0]
    theirs = composition(log_w, loc, target, scale, u, rows)
    agree = float((mine == theirs).double().mean())
    kernel = timed(lambda: k.backward_sample(log_w, loc, target, scale, u), 3, 21)
    torch_ = timed(lambda: composition(log_w, loc, target, scale, u, rows), 1, 5)
    pairs = B * K * M
    flops = pairs * (8 * D + 7 + EXP_FLOPS)      # two passes of (sub, mul, fma) per d, the score, max / sum, one exp
    print("B={} K={} M={} D={} float32: {:.3e} pairs, {:.3e} float64 operations; us, median (min .. max)".format(
        B, K, M, D, pairs, flops))
    print("  kernel K21                 {:10.1f} ({:.1f} .. {:.1f})   {:.2f} TFLOP/s = {:.1f} % of the float64 vector peak".format(
        *kernel, flops / kernel[0] / 1e6, 100 * flops / kernel[0] / 1e-6 / PEAK_FP64_VECTOR))
    print("  PyTorch float64 composition {:9.1f} ({:.1f} .. {:.1f})   {} trajectories per chunk".format(*torch_, rows))
    print("  composition / kernel at the medians: {:.1f}x; indices equal: {:.6f}".format(torch_[0] / kernel[0], agree),
          flush=True)
