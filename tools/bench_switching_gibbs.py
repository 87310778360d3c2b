"""K37 (aesmc_switching_conditional_ancestor_index) beside the composition it replaces, on the same device inputs: K35 with
one trajectory per batch row (aesmc_switching_backward_scores, N = 1), K26 without a transition term
(aesmc_conditional_ancestor_index), K21's draw on the scores (aesmc_backward_sample) and the scatter of its index into column
K-1.  Timed warm between HIP events, the median per call with the spread; the two are checked to give the same indices first.
Then K38 (aesmc_switching_kalman_conditional_step) beside K31, and a whole sweep of `conditional_switching_filter`.
    python tools/bench_switching_gibbs.py [--out FILE] [B,K,M,D,Dy ...]
(default: B = 1024, K = 64 and 1024, D = Dy = 4 and 8; the report goes to profiles/switching_gibbs.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels, rao_blackwell  # noqa: E402
from aesmc_amd.testing import rao_blackwell as contract  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def timed(fn, warm, reps, run):
    """(median, min, max) in microseconds per call: `run` back-to-back calls between two events, after one untimed call."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(run):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / run)
    return sorted(times)[len(times) // 2], min(times), max(times)


def kernels(lines, B, K, M, D, Dy):
    model = contract.example_model(M, D, Dy, seed=1)
    ops = {name: torch.from_numpy(np.array(value)).to(dev) for name, value in model.items()}
    log_Pi = torch.log(ops["Pi"])
    gen = torch.Generator(device=dev).manual_seed(1)
    regime = torch.randint(0, M, (B, K), generator=gen, device=dev, dtype=torch.int32)
    mean = torch.randn(B, K, D, generator=gen, device=dev, dtype=torch.float64)
    factor = torch.randn(B, K, D, D, generator=gen, device=dev, dtype=torch.float64)
    full = factor @ factor.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64)
    rows, cols = torch.tril_indices(D, D, device=dev)
    state = (regime, mean, full[..., rows, cols].contiguous())
    del factor, full
    log_w = torch.randn(B, K, generator=gen, device=dev, dtype=torch.float64)
    u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
    y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
    nexts = [torch.randint(0, M, (B, 1), generator=gen, device=dev, dtype=torch.int32) for _ in range(3)]
    info = None
    for regime_next in nexts[:2]:      # two steps from the zeros: a full-rank Om, as most steps of a sweep see
        om, lam, c, F = k.switching_information_step(ops, regime_next, info, y)
        info = (om, lam, c)
    regime_next = nexts[2]
    om, lam, c, F = k.switching_information_step(ops, regime_next, info, y)
    pinned_regime, F1, lam1 = regime_next[:, 0].contiguous(), F[:, 0].contiguous(), lam[:, 0].contiguous()
    u_last = u[:, K - 1:].contiguous()

    def fused():
        return k.switching_conditional_ancestor_index(log_w, u, log_Pi, pinned_regime, F1, lam1, state)

    def composed():
        scores = k.switching_backward_scores(log_Pi, regime_next, F, lam, state, log_w)
        index = k.conditional_ancestor_index(log_w, u)
        drawn, _ = k.backward_sample(scores[:, 0, :], None, None, None, u_last)
        index[:, K - 1] = drawn[:, 0]
        return index

    same = bool(torch.equal(fused(), composed()))
    flags = k.read_flags(dev)
    t_fused = timed(fused, 3, 10, 8)
    t_composed = timed(composed, 3, 10, 8)
    t_plain = timed(lambda: k.switching_conditional_ancestor_index(log_w, u, log_Pi, pinned_regime, None, None, state), 3, 10, 8)
    t_k26 = timed(lambda: k.conditional_ancestor_index(log_w, u), 3, 10, 8)
    t_k35 = timed(lambda: k.switching_backward_scores(log_Pi, regime_next, F, lam, state, log_w), 3, 10, 8)
    regime_u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
    index = fused().clamp(max=K - 1)
    t_k38 = timed(lambda: k.switching_kalman_conditional_step(ops, state, index, regime_u, pinned_regime, y), 3, 10, 8)
    t_k31 = timed(lambda: k.switching_kalman_step(ops, state, index, regime_u, y), 3, 10, 8)
    flags |= k.read_flags(dev)
    lines.append("B={} K={} M={} D={} Dy={} (flags {}; K37 and the composition give the same indices: {})".format(
        B, K, M, D, Dy, flags, same))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("K37, one launch", *t_fused))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us   K37 takes {:.2f} of it".format(
        "K35 (N = 1) + K26 + K21 + the scatter", *t_composed, t_fused[0] / t_composed[0]))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("  of which K35 with N = 1", *t_k35))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("  of which K26 without a transition term", *t_k26))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("K37 without ancestor sampling", *t_plain))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us   K31: {:.1f} ({:.1f} .. {:.1f}) us".format(
        "K38 conditional step", *t_k38, *t_k31))
    torch.cuda.empty_cache()


def sweep(lines, B=1024, K=64, T=100):
    ops, series = contract.sticky_example(T=T, seed=0)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(dev)
    ys = [torch.from_numpy(np.broadcast_to(y, (B, y.shape[0])).copy()).to(dev) for y in series]
    reference = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(T)]
    torch.manual_seed(3)
    for ancestor_sampling in (True, False):
        t = timed(lambda: rao_blackwell.conditional_switching_filter(ys, model, K, reference,
                                                                     ancestor_sampling=ancestor_sampling), 1, 5, 1)
        lines.append("one sweep of conditional_switching_filter, contract.sticky_example (M=3, D=Dy=1), T={}, B={}, K={}, "
                     "ancestor_sampling={}: {:.1f} ({:.1f} .. {:.1f}) us, host included".format(T, B, K, ancestor_sampling, *t))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "switching_gibbs.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or \
        [(1024, 64, 4, 4, 4), (1024, 1024, 4, 4, 4), (1024, 64, 4, 8, 8), (1024, 1024, 4, 8, 8)]
    lines = ["tools/bench_switching_gibbs.py on one {} ({}), float64 throughout, float32 observations, HIP events, warm; us per "
             "call through the provider (allocation and launch latency included): median (min .. max)".format(
                 torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for shape in shapes:
        kernels(lines, *shape)
    sweep(lines)
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
