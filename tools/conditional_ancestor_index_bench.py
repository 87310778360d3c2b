"""The conditional-resampling launch (aesmc_conditional_ancestor_index, K26) beside the two-launch composition of K21
(aesmc_backward_sample) it replaces: the free slots as `backward_sample` without a transition term and M = K - 1
trajectories, the pinned slot as `backward_sample` with M = 1.  Both are timed warm between HIP events around a run of
launches issued back to back (one synchronisation per run), the two alternating; the median over the runs is reported per
launch (per pair of launches) with the spread.
    python tools/conditional_ancestor_index_bench.py [--out FILE] [B,K,D ...]
    (default: 1024,64,10  1024,512,10  1024,4096,10; float32; FILE defaults to profiles/conditional_ancestor_index.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()


def run_of(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "conditional_ancestor_index.txt")
    if argv[:1] == ["--out"]:
        out_path, argv = argv[1], argv[2:]
    lines = ["K26 (aesmc_conditional_ancestor_index) beside the two K21 launches it replaces; float32 operands, one MI355X;",
             "us per call: median (min .. max) over runs of back-to-back launches between HIP events, the two alternating"]
    for spec in argv or ["1024,64,10", "1024,512,10", "1024,4096,10"]:
        B, K, D = [int(v) for v in spec.split(",")]
        gen = torch.Generator(device=dev).manual_seed(0)
        log_w = torch.randn(B, K, device=dev, generator=gen)
        loc = torch.randn(B, K, D, device=dev, generator=gen)
        target = torch.randn(B, D, device=dev, generator=gen)
        scale = torch.full((1,), 0.9, device=dev)
        u = torch.rand(B, K, device=dev, dtype=torch.float64, generator=gen)
        u_free, u_pinned, target_one = u[:, :K - 1].contiguous(), u[:, K - 1:].contiguous(), target[:, None]

        def kernel():
            return k.conditional_ancestor_index(log_w, u, loc, target, scale)

        def composition():
            free = k.backward_sample(log_w, None, None, None, u_free)[0]
            pinned = k.backward_sample(log_w, loc, target_one, scale, u_pinned)[0]
            return free, pinned

        mine, (free, pinned) = kernel(), composition()
        agree = float((mine == torch.cat([free, pinned], dim=1)).double().mean())
        torch.cuda.synchronize()
        # runs of about a tenth of a second of device work for the composition, never fewer than 3 launches
        probe = run_of(composition, 1)
        launches_c = max(3, min(200, int(1e5 / max(probe, 1.0))))
        launches_k = 200
        run_of(kernel, 20), run_of(composition, 2)
        times_k, times_c = [], []
        for _ in range(7):
            times_k.append(run_of(kernel, launches_k))
            times_c.append(run_of(composition, launches_c))
        times_k.sort(), times_c.sort()
        mk, mc = times_k[len(times_k) // 2], times_c[len(times_c) // 2]
        lines.append("B={} K={} D={}: K26 {:.1f} ({:.1f} .. {:.1f}) us, {} launches per run;  K21 + K21 {:.1f} ({:.1f} .. {:.1f}) "
                     "us, {} pairs per run;  composition / K26 = {:.1f}x;  indices equal: {:.6f}".format(
                         B, K, D, mk, times_k[0], times_k[-1], launches_k, mc, times_c[0], times_c[-1], launches_c,
                         mc / mk, agree))
        print(lines[-1], flush=True)
    assert k.read_flags(dev) == 0
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
