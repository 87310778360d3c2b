"""K50 (aesmc_switching_collapse) and K51 (aesmc_switching_pair_smooth) alone, and one whole pass of the collapsed-mixture filter
of each order and of Kim's smoother beside `adapted_switching_filter` on the same series: timed warm between HIP events, the
median with the spread.  No thresholds: these launches are small and bound by launch cost.
    python tools/bench_switching_collapsed.py [--out FILE] [--batch 1024] [--regimes 4] [--timesteps 100] [--particles 256]
(the report goes to profiles/switching_collapsed.txt)"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels, rao_blackwell  # noqa: E402
from aesmc_amd.testing import rao_blackwell as contract  # noqa: E402
from aesmc_amd.testing import switching_collapsed as collapsed  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def timed(fn, warm, reps, run=1):
    """(median, min, max) in microseconds per call: `run` back-to-back calls between two events, after `warm` untimed ones."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(run):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / run)
    return sorted(times)[len(times) // 2], min(times), max(times)


def kernel_report(lines, B, M, D):
    to = lambda array: torch.from_numpy(array).to(dev)
    mean, cov, lw = (to(part) for part in collapsed.example_collapse(B, M, M, D))
    model, m, P, ms, Ps = collapsed.example_pair_smooth(B, M, D, D)
    ops = {name: to(value) for name, value in model.items()}
    m, P, ms, Ps = to(m), to(P), to(ms), to(Ps)
    shared_mean, shared_cov = mean[:, 0].contiguous(), cov[:, 0].contiguous()
    one_mean, one_cov, one_lw = mean[:, :1].contiguous(), cov[:, :1].contiguous(), lw[:, :1].contiguous()
    rows = (("K50 dense  [B,M,M]: a step's collapse of the pairs", lambda: k.switching_collapse(mean, cov, lw)),
            ("K50 shared [B,M,M]: IMM's mixing", lambda: k.switching_collapse(shared_mean, shared_cov, lw)),
            ("K50 dense  [B,1,M]: the overall moments", lambda: k.switching_collapse(one_mean, one_cov, one_lw)),
            ("K51 [B,M,M]: the pair-smoothed components", lambda: k.switching_pair_smooth(ops, m, P, ms, Ps)))
    lines.append("B={} M={} D=Dy={}: one launch, 8 back to back, output allocation included".format(B, M, D))
    for label, fn in rows:
        lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format(label, *timed(fn, 3, 15, 8)))


def pass_report(lines, B, M, D, T, K):
    model = rao_blackwell.SwitchingLinearGaussian(*[contract.example_model(M, D, D, seed=1)[key] for key in KEYS]).to(dev)
    observations = model.simulate(T, B, seed=1)
    rows = (("collapsed_switching_filter order 2 (GPB2 / Kim)", lambda: rao_blackwell.collapsed_switching_filter(observations, model, 2)),
            ("collapsed_switching_filter order 1 (IMM)", lambda: rao_blackwell.collapsed_switching_filter(observations, model, 1)),
            ("collapsed_switching_smooth (Kim's smoother)", lambda: rao_blackwell.collapsed_switching_smooth(observations, model)),
            ("adapted_switching_filter K={}".format(K), lambda: rao_blackwell.adapted_switching_filter(observations, model, K)))
    lines.append("B={} M={} D=Dy={} T={}: one whole pass, the read of the flags at its end included".format(B, M, D, T))
    evidence = []
    for label, fn in rows:
        evidence.append(fn()["log_marginal_likelihood"].mean().item() / T)
        lines.append("  {:<52} {:9.2f} ({:.2f} .. {:.2f}) ms   log evidence per step {:.5f}".format(
            label, *[value / 1e3 for value in timed(fn, 1, 5)], evidence[-1]))


def main(argv):
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "switching_collapsed.txt"))
    parser.add_argument("--batch", type=int, default=1024)
    parser.add_argument("--regimes", type=int, default=4)
    parser.add_argument("--timesteps", type=int, default=100)
    parser.add_argument("--particles", type=int, default=256)
    args = parser.parse_args(argv)
    lines = ["tools/bench_switching_collapsed.py on one {} ({}), float64 throughout, HIP events, warm, host time of the launches "
             "included: median (min .. max)".format(torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for D in (4, 8):
        kernel_report(lines, args.batch, args.regimes, D)
    for D in (4, 8):
        pass_report(lines, args.batch, args.regimes, D, args.timesteps, args.particles)
    assert k.read_flags(dev) == 0
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
