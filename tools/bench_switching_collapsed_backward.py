"""The differentiable collapsed-mixture evidence, timed: the forward pass alone (`collapsed_switching_filter`, what the pass
cost before it had a gradient, and `collapsed_switching_log_likelihood` with the tape), forward + backward through K52 / K54,
the same forward + backward as the plain-torch float64 restatement on the same device (the composition the kernels replace),
and K52 and K54 per launch.  Warm, between HIP events, the median with the spread.  No thresholds.
    python tools/bench_switching_collapsed_backward.py [--out FILE] [--batch 1024] [--regimes 4] [--timesteps 100]
Every section runs in a child process of its own under its own time limit; the first one that fails ends the run.
(the report goes to profiles/switching_collapsed_backward.txt)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
SECTIONS = (("kernels", 120), ("pass", 240), ("restated", 420))      # name, seconds


def timed(fn, warm, reps, run=1):
    """(median, min, max) in microseconds per call: `run` back-to-back calls between two events, after `warm` untimed ones."""
    import torch
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


def section(name, B, M, T, D):
    import torch
    sys.path.insert(0, ROOT)
    import aesmc_amd  # noqa: F401
    from aesmc_amd import _kernels, rao_blackwell
    from aesmc_amd.testing import rao_blackwell as contract
    from aesmc_amd.testing import switching_collapsed as collapsed
    from aesmc_amd.testing import switching_collapsed_backward as backward
    dev = torch.device("cuda", 0)
    k = _kernels.get()
    to = lambda array: torch.from_numpy(array).to(dev)
    lines = []
    if name == "kernels":
        args = backward.example_step_backward(B, M * M, M, D, D)
        ops = {key: to(value) for key, value in args[0].items()}
        regime, mean, cov, y, g_mean, g_cov, g_lw = [to(args[1])] + [to(part) for part in args[2]] + [to(x) for x in args[3:7]]
        every = ("A", "b", "q", "C", "d", "r")
        step = lambda need_state, need: k.switching_kalman_step_backward(ops, regime, (mean, cov), y, g_mean, g_cov, g_lw,
                                                                         need_state=need_state, need=need)
        pairs = tuple(to(part) for part in collapsed.example_collapse(B, M, M, D))
        arriving = tuple(to(part) for part in backward.example_collapse_backward(B, M, M, D))
        shared = (pairs[0][:, 0].contiguous(), pairs[1][:, 0].contiguous(), pairs[2])
        rows = (("K52 [B,M^2]: per-slot and per-regime gradients (+ finish)", lambda: step(True, every)),
                ("K52 [B,M^2]: per-slot gradients only", lambda: step(True, ())),
                ("K52 [B,M^2]: per-regime gradients only (+ finish)", lambda: step(False, every)),
                ("K31 [B,M^2]: the forward step, for scale", lambda: k.switching_kalman_step(
                    ops, (regime, mean, cov), None, (regime.double() + 0.5) / M, y)),
                ("K54 dense  [B,M,M]", lambda: k.switching_collapse_backward(*pairs, *arriving)),
                ("K54 shared [B,M,M]", lambda: k.switching_collapse_backward(*shared, *arriving)),
                ("K50 dense  [B,M,M]: the forward collapse, for scale", lambda: k.switching_collapse(*pairs)))
        lines.append("B={} M={} D=Dy={}: one launch, 8 back to back, output and workspace allocation included".format(B, M, D))
        for label, fn in rows:
            lines.append("  {:<60} {:9.1f} ({:.1f} .. {:.1f}) us".format(label, *timed(fn, 3, 15, 8)))
    else:
        truth = contract.example_model(M, D, D, seed=1)
        model = rao_blackwell.SwitchingLinearGaussian(*[truth[key] for key in KEYS]).to(dev)
        observations = model.simulate(T, B, seed=1)
        leaves = {key: to(truth[key].copy()).requires_grad_(True) for key in KEYS}

        def both(function):
            loss = -function(observations, leaves).mean()
            return torch.autograd.grad(loss, list(leaves.values()))

        if name == "pass":
            rows = (("collapsed_switching_filter (no tape: the pass as it was)",
                     lambda: rao_blackwell.collapsed_switching_filter(observations, model, 2)),
                    ("collapsed_switching_log_likelihood, forward with the tape",
                     lambda: rao_blackwell.collapsed_switching_log_likelihood(observations, leaves)),
                    ("collapsed_switching_log_likelihood, forward + backward",
                     lambda: both(rao_blackwell.collapsed_switching_log_likelihood)))
        else:
            rows = (("plain-torch float64 restatement, forward + backward",
                     lambda: both(backward.collapsed_log_likelihood_restated)),)
        lines.append("B={} M={} D=Dy={} T={} order 2: one whole pass".format(B, M, D, T))
        for label, fn in rows:
            lines.append("  {:<60} {:9.2f} ({:.2f} .. {:.2f}) ms".format(label, *[v / 1e3 for v in timed(fn, 1, 5)]))
        if name == "pass":
            mine = both(rao_blackwell.collapsed_switching_log_likelihood)
            theirs = both(backward.collapsed_log_likelihood_restated)
            worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(mine, theirs))
            lines.append("  largest relative difference of the ten gradients from the restatement's: {:.2e}".format(worst))
    assert k.read_flags(dev) == 0
    print("\n".join(lines))


def main(argv):
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "switching_collapsed_backward.txt"))
    parser.add_argument("--batch", type=int, default=1024)
    parser.add_argument("--regimes", type=int, default=4)
    parser.add_argument("--timesteps", type=int, default=100)
    parser.add_argument("--section", default=None)
    parser.add_argument("--dim", type=int, default=4)
    args = parser.parse_args(argv)
    if args.section is not None:
        section(args.section, args.batch, args.regimes, args.timesteps, args.dim)
        return 0
    report = ["tools/bench_switching_collapsed_backward.py on one MI355X (gfx950), float64 throughout, HIP events, warm, host "
              "time of the launches included: median (min .. max)"]
    for D in (4, 8):
        for name, seconds in SECTIONS:
            command = [sys.executable, os.path.abspath(__file__), "--section", name, "--dim", str(D), "--batch", str(args.batch),
                       "--regimes", str(args.regimes), "--timesteps", str(args.timesteps)]
            try:
                done = subprocess.run(command, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=seconds, text=True)
            except subprocess.TimeoutExpired:
                print("section {} at D = {} ran past its {} s: stopping".format(name, D, seconds))
                return 1
            print(done.stdout, end="", flush=True)
            if done.returncode != 0:
                print("section {} at D = {} failed with status {}: stopping".format(name, D, done.returncode))
                return 1
            report.append(done.stdout.rstrip("\n"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as handle:
        handle.write("\n".join(report) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
