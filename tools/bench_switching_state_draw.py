"""K47 (aesmc_switching_state_draw) — the whole backward pass of the simulation smoother in one launch — beside the same
arithmetic as a plain-torch route, per timestep `torch.linalg.cholesky` / `solve_triangular` on [B N, D, D]: timed warm between
HIP events, the median per pass with the spread, and the peak memory each route allocates.  Both routes start from the
conditional filter's moments as `conditional_kalman_filter` returns them (T tensors per operand).
    python tools/bench_switching_state_draw.py [--out FILE] [B,N,T,M,D,Dy ...]
(default: 16,128,100,2,2,2 and 16,128,100,16,8,8, profiles/switching_statistics.txt's shapes; the report goes to
profiles/switching_state_draw.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels, rao_blackwell  # noqa: E402
from aesmc_amd.testing import rao_blackwell as contract  # noqa: E402

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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def torch_state_draw(ops, regimes, means, covs, noise, D):
    """The backward pass in plain torch on nonsingular inputs (no pivot is dropped): per timestep the gathers of A, b, q by
    regime, S = A P A^T + Q, its factor, two triangular solves, the downdate, its factor and the draw."""
    T = len(means)
    lower = lambda packed: rao_blackwell.unpack_covariance(packed, D)
    states = [None] * T
    states[T - 1] = means[T - 1] + (torch.linalg.cholesky(lower(covs[T - 1])) @ noise[T - 1].unsqueeze(-1)).squeeze(-1)
    for t in range(T - 2, -1, -1):
        j = regimes[t + 1].long()
        A, b, q = ops["A"][j], ops["b"][j], ops["q"][j]
        P, m = lower(covs[t]), means[t]
        V = A @ P
        S = V @ A.transpose(-1, -2) + torch.diag_embed(q * q)
        L = torch.linalg.cholesky(S)
        e = states[t + 1] - b - (A @ m.unsqueeze(-1)).squeeze(-1)
        U = torch.linalg.solve_triangular(L, V, upper=False)
        v = torch.linalg.solve_triangular(L, e.unsqueeze(-1), upper=False)
        factor = torch.linalg.cholesky(P - U.transpose(-1, -2) @ U)
        states[t] = m + (U.transpose(-1, -2) @ v).squeeze(-1) + (factor @ noise[t].unsqueeze(-1)).squeeze(-1)
    return states


def shape_report(lines, B, N, T, M, D, Dy):
    model = rao_blackwell.SwitchingLinearGaussian(*[contract.example_model(M, D, Dy, seed=1)[key] for key in KEYS]).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    observations = model.simulate(T, B, seed=1)
    regimes = [torch.randint(0, M, (B, N), generator=gen, device=dev, dtype=torch.int32) for _ in range(T)]
    noise = [torch.randn(B, N, D, generator=gen, device=dev, dtype=torch.float64) for _ in range(T)]
    filtered = rao_blackwell.conditional_kalman_filter(observations, model, regimes)
    means, covs = filtered["means"], filtered["covariances"]
    ops = model.operands()
    stacked = [torch.stack(part) for part in (regimes, means, covs, noise)]
    with_stacks = lambda: k.switching_state_draw(ops, torch.stack(regimes), torch.stack(means), torch.stack(covs), torch.stack(noise))
    alone = lambda: k.switching_state_draw(ops, *stacked)
    plain = lambda: torch_state_draw(ops, regimes, means, covs, noise, D)
    states, again, reference = with_stacks(), alone(), torch.stack(plain())
    assert k.read_flags(dev) == 0
    difference = float((states - reference).abs().max())
    t_stacks, t_alone, t_torch = timed(with_stacks, 3, 15), timed(alone, 3, 15, 8), timed(plain, 2, 9)
    m_stacks, m_alone, m_torch = peak_bytes(with_stacks), peak_bytes(alone), peak_bytes(plain)
    lines.append("B={} N={} T={} M={} D={} Dy={}: largest |kernel - torch| over the states {:.2e}; the kernel twice gives the same "
                 "bits: {}".format(B, N, T, M, D, Dy, difference, torch.equal(states, again)))
    lines.append("  {:<44} {:10.1f} ({:.1f} .. {:.1f}) us   peak {:8.2f} MB".format(
        "K47 pass, four torch.stack + one launch", *t_stacks, m_stacks / 1e6))
    lines.append("  {:<44} {:10.1f} ({:.1f} .. {:.1f}) us   peak {:8.2f} MB   8 back to back".format(
        "K47 alone (operands already stacked)", *t_alone, m_alone / 1e6))
    lines.append("  {:<44} {:10.1f} ({:.1f} .. {:.1f}) us   peak {:8.2f} MB   the kernel route takes {:.3f} of its time".format(
        "plain torch, per timestep linalg", *t_torch, m_torch / 1e6, t_stacks[0] / t_torch[0]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "switching_state_draw.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or [(16, 128, 100, 2, 2, 2), (16, 128, 100, 16, 8, 8)]
    lines = ["tools/bench_switching_state_draw.py on one {} ({}), float64 throughout, HIP events, warm; us per backward pass over T "
             "timesteps of B N trajectories, host time of the launches included: median (min .. max)".format(
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
