"""The two launches of the pairwise weighted pass (aesmc_pairwise_pass, K25) that make the backward of the pairwise
log-sum-exp — the row points own the columns (pull, with and without spread), the columns own the row points (mass and
pull) — beside the forward launch (aesmc_pairwise_lse, K22) on the same operands and beside the BACKWARD of the PyTorch
float64 composition of the same contract on the same device (a broadcast difference, sum and logsumexp under autograd,
chunked over the row points so that its [B, r, C, D] float64 intermediates fit in memory).  Everything is timed warm
between HIP events, one launch (one composition) per pair of events, the launches alternating within each repetition; the
median is reported with the spread.  Operations are the ALGORITHM's (K22's 4 D + 39 per pair, plus 5 D for pull and 1 D
more for spread), so the share of the float64 vector peak compares the launches directly.
    python tools/pairwise_pass_bench.py [B,N,D ...]        (N = M; default: 64,1024,10 and 1024,512,10; float64 operands,
                                                            as `_ops.pairwise_lse` launches its backward)"""
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


def composition_backward(rows, cols, scale, col_a, grad, chunk):
    """Forward and backward of the explicit composition under autograd, chunk by chunk: gradients of rows, cols, col_a."""
    rows, cols, col_a = (t.detach().requires_grad_(True) for t in (rows, cols, col_a))
    inv = 1.0 / scale
    for r0 in range(0, rows.shape[1], chunk):
        diff = (rows[:, r0:r0 + chunk, None, :] - cols[:, None, :, :]) * inv
        out = torch.logsumexp(col_a[:, None, :] - 0.5 * (diff * diff).sum(-1), dim=-1)
        out.backward(grad[:, r0:r0 + chunk])
    return rows.grad, cols.grad, col_a.grad


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


print("tools/pairwise_pass_bench.py on one {} ({}), float64 operands, HIP events, warm".format(
    torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode()))
for spec in sys.argv[1:] or ["64,1024,10", "1024,512,10"]:
    B, N, D = [int(v) for v in spec.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device=dev, generator=gen, dtype=torch.float64)
    rows, cols, col_a, grad = rand(B, N, D), rand(B, N, D), rand(B, N), rand(B, N)
    scale = torch.full((1,), 0.9, device=dev, dtype=torch.float64)
    out = k.pairwise_lse(rows, cols, scale, col_a)
    minus_l = -out
    pairs = B * N * N
    score = 4 * D + 5 + EXP_FLOPS
    launches = [
        ("K22 forward (pairwise_lse)", score, lambda: k.pairwise_lse(rows, cols, scale, col_a)),
        ("K25 rows side: pull", score + 5 * D, lambda: k.pairwise_pass(
            rows, cols, scale, minus_l, col_a, own_gain=grad, want_mass=False, want_pull=True, want_spread=False)),
        ("K25 rows side: pull and spread", score + 6 * D, lambda: k.pairwise_pass(
            rows, cols, scale, minus_l, col_a, own_gain=grad, want_mass=False, want_pull=True, want_spread=True)),
        ("K25 cols side: mass and pull", score + 5 * D, lambda: k.pairwise_pass(
            cols, rows, scale, col_a, minus_l, other_gain=grad, want_mass=True, want_pull=True, want_spread=False)),
        ("K25 cols side: mass alone", score, lambda: k.pairwise_pass(
            cols, rows, scale, col_a, minus_l, other_gain=grad, want_mass=True, want_pull=False, want_spread=False)),
    ]
    chunk = max(1, min(N, (1 << 31) // (B * N * D * 8)))      # 2 GiB for the [B, chunk, N, D] float64 difference
    print("B={} N=M={} D={} float64: {:.3e} pairs; us, median (min .. max)".format(B, N, D, pairs))
    theirs = composition_backward(rows, cols, scale, col_a, grad, chunk)
    _, pull_rows, _ = launches[1][2]()
    mass_cols, pull_cols, _ = launches[3][2]()
    for name, mine, reference in (("rows", pull_rows, theirs[0]), ("cols", pull_cols, theirs[1]), ("col_a", mass_cols, theirs[2])):
        print("  largest difference from the composition's gradient of {:5s} {:.1e} (largest magnitude {:.1e})".format(
            name, float((mine - reference).abs().max()), float(reference.abs().max())))
    reps = 5 if pairs > 1e10 else 21
    results = timed([fn for _, _, fn in launches], 2, reps)
    torch_ = timed([lambda: composition_backward(rows, cols, scale, col_a, grad, chunk)], 1, 3)[0]
    for (name, per_pair, _), result in zip(launches, results):
        flops = pairs * per_pair
        print("  {:32s} {:10.1f} ({:.1f} .. {:.1f})   {:5.2f} TFLOP/s = {:4.1f} % of the float64 vector peak; {:.2f}x the "
              "forward".format(name, *result, flops / result[0] / 1e6, 100 * flops / result[0] / 1e-6 / PEAK_FP64_VECTOR,
                               result[0] / results[0][0]))
    both = results[1][0] + results[3][0]
    print("  PyTorch float64 composition, forward and backward {:10.1f} ({:.1f} .. {:.1f})   {} row points per chunk".format(
        *torch_, chunk))
    print("  composition / (K22 + the two K25 launches of a backward without the scale) at the medians: {:.1f}x".format(
        torch_[0] / (results[0][0] + both)), flush=True)
