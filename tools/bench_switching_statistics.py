"""K45 (aesmc_switching_moment_statistics) with its finishing launch — the reduction from per-trajectory smoothed moments to
the expected sufficient statistics of a switching model — beside the plain-torch route to the same sums that
examples/slds_em.py's `m_step` takes (the stacked second moments, `index_put_` for the transition counts, a masked sum per
regime): timed warm between HIP events, the median per pass with the spread, and the peak memory each route allocates.
    python tools/bench_switching_statistics.py [--out FILE] [B,N,T,M,D,Dy ...]
(default: 16,128,100,2,2,2 — the example's shape — and 16,128,100,16,8,8; the report goes to profiles/switching_statistics.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels, rao_blackwell  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def torch_statistics(out, M, D):
    """The sums examples/slds_em.py's M-step forms, for every regime: transition counts, and per regime j the totals over the
    steps with s_{t+1} = j of E[z_t z_t^T], E[z_t], E[z_{t+1} z_t^T], E[z_{t+1}] and the count."""
    regimes = torch.stack(out["regimes"]).long()
    means = torch.stack(out["means"])
    second = rao_blackwell.unpack_covariance(torch.stack(out["covariances"]), D) + means.unsqueeze(-1) * means.unsqueeze(-2)
    lagged = torch.stack(out["cross_covariances"]) + means[1:].unsqueeze(-1) * means[:-1].unsqueeze(-2)
    counts = torch.zeros(M, M, dtype=torch.float64, device=means.device)
    counts.index_put_((regimes[:-1].reshape(-1), regimes[1:].reshape(-1)),
                      torch.ones(regimes[1:].numel(), dtype=torch.float64, device=means.device), accumulate=True)
    sums = []
    for j in range(M):
        w = (regimes[1:] == j).to(torch.float64)
        total = lambda x: (w.reshape(w.shape + (1,) * (x.dim() - 3)) * x).sum(dim=(0, 1, 2))
        sums.append((total(second[:-1]), total(means[:-1]), total(lagged), total(means[1:]), w.sum()))
    return counts, sums


def shape_report(lines, B, N, T, M, D, Dy):
    gen = torch.Generator(device=dev).manual_seed(1)
    rows, cols = torch.tril_indices(D, D, device=dev)

    def packed():
        root = torch.randn(B, N, D, D, generator=gen, device=dev, dtype=torch.float64)
        return (root @ root.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64))[..., rows, cols].contiguous()

    out = {"regimes": [torch.randint(0, M, (B, N), generator=gen, device=dev, dtype=torch.int32) for _ in range(T)],
           "means": [torch.randn(B, N, D, generator=gen, device=dev, dtype=torch.float64) for _ in range(T)],
           "covariances": [packed() for _ in range(T)],
           "cross_covariances": [0.3 * torch.randn(B, N, D, D, generator=gen, device=dev, dtype=torch.float64) for _ in range(T - 1)]}
    observations = [torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float64) for _ in range(T)]
    kernel = lambda: rao_blackwell.switching_expected_statistics(out, observations, M)
    plain = lambda: torch_statistics(out, M, D)
    statistics, (counts, sums) = kernel(), plain()
    again = kernel()
    same = all(torch.equal(statistics[name], again[name]) for name in statistics if torch.is_tensor(statistics[name]))
    difference = max(float((statistics["transition_counts"] - counts).abs().max()),
                     max(float((statistics["next_prev"][j, :, :D] - sums[j][2]).abs().max()) for j in range(M)))
    t_kernel, t_torch = timed(kernel, 2, 9), timed(plain, 2, 9)
    m_kernel, m_torch = peak_bytes(kernel), peak_bytes(plain)
    earlier = (out["regimes"][0], out["means"][0], out["covariances"][0], out["cross_covariances"][0])
    t_step = timed(lambda: k.switching_statistics_step(observations[1], out["regimes"][1], out["means"][1], out["covariances"][1],
                                                       M, previous=earlier, block=1), 3, 9, 32)
    lines.append("B={} N={} T={} M={} D={} Dy={}: largest |kernel - torch| over the counts and E[z_t+1 z_t^T] {:.2e}; the kernel "
                 "route twice gives the same bits: {}".format(B, N, T, M, D, Dy, difference, same))
    lines.append("  {:<44} {:10.1f} ({:.1f} .. {:.1f}) us   peak {:8.2f} MB".format(
        "K45 per timestep + two finishes (all sums)", *t_kernel, m_kernel / 1e6))
    lines.append("  {:<44} {:10.1f} ({:.1f} .. {:.1f}) us   per launch, 32 back to back".format("K45 alone (a later step)", *t_step))
    lines.append("  {:<44} {:10.1f} ({:.1f} .. {:.1f}) us   peak {:8.2f} MB   the kernel route takes {:.2f} of its time".format(
        "plain torch (counts, A and b's sums only)", *t_torch, m_torch / 1e6, t_kernel[0] / t_torch[0]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "switching_statistics.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or [(16, 128, 100, 2, 2, 2), (16, 128, 100, 16, 8, 8)]
    lines = ["tools/bench_switching_statistics.py on one {} ({}), float64 throughout, HIP events, warm; us per pass over T "
             "timesteps, host time of the launches included: median (min .. max)".format(
                 torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for shape in shapes:
        shape_report(lines, *shape)
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
