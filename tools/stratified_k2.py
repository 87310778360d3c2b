"""The stratified resampling launch beside the systematic one (aesmc_resample_step_ranges, the headline route) and the
torch.rand that draws its [B,K] float64 uniforms: hipGraph-timed between HIP events on six operand sets of N(0,1)
log-weights, the three alternating over several rounds so that the run-to-run spread is on the page.
    python tools/stratified_k2.py [B,K ...]        (default: 1024,4096)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
SETS, ROUNDS = 6, 5


def timeit(fn, replays=5):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(SETS):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for rep in range(3):
            for i in range(SETS):
                fn(i)
    graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (3 * SETS * replays)


for spec in sys.argv[1:] or ["1024,4096"]:
    B, K = [int(v) for v in spec.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    lw = [torch.randn(B, K, device=dev, generator=gen) for _ in range(SETS)]
    u_row = torch.rand(B, device=dev, dtype=torch.float64, generator=gen)
    u_all = [torch.rand(B, K, device=dev, dtype=torch.float64, generator=gen) for _ in range(SETS)]
    legs = (
        ("systematic, ranges + lse", 16, lambda i: k.resample_step(lw[i], u_row, None, True, want_child_end=True)),
        ("stratified, ranges + lse", 24, lambda i: k.resample_step(lw[i], u_all[i], None, True, want_child_end=True)),
        ("torch.rand [B,K] float64", 8, lambda i: torch.rand(B, K, device=dev, dtype=torch.float64)),
    )
    print("B={} K={} float32 log-weights; us per launch, {} rounds alternating".format(B, K, ROUNDS), flush=True)
    times = {name: [] for name, _, _ in legs}
    for _ in range(ROUNDS):
        for name, _, fn in legs:
            times[name].append(timeit(fn))
    for name, per_particle, _ in legs:
        t = sorted(times[name])
        nbytes = B * K * per_particle
        print("  {:26s} median {:7.1f}  min {:7.1f}  max {:7.1f}   {:6.1f} MB  {:5.2f} TB/s at the median".format(
            name, t[len(t) // 2], t[0], t[-1], nbytes / 1e6, nbytes / t[len(t) // 2] / 1e6), flush=True)
    ratio = sorted(times[legs[1][0]])[ROUNDS // 2] / sorted(times[legs[0][0]])[ROUNDS // 2]
    print("  stratified / systematic at the medians: {:.2f}".format(ratio), flush=True)
