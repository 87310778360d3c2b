"""K48 (aesmc_switching_lookahead_conditional_ancestor_index) beside the composition it replaces, on the same device inputs:
K32 (aesmc_switching_lookahead), K37 on the first-stage weights, K37 on zeros for the pinned slot and one torch.where.  Timed
warm between HIP events, the median per call with the spread; the two are checked to give the same indices first.  Then a
whole sweep of `conditional_switching_filter` with and without lookahead in the same run, and what the look-ahead buys: the
share of time points whose regime a sweep changes and the integrated autocorrelation time of the regime indicator along the
chain, look-ahead against bootstrap, on a mild and on an abrupt series.
    python tools/bench_switching_lookahead_gibbs.py [--out FILE] [B,K,M,D,Dy ...]
(default: B = 1024, M = 4, K = 8, 64 and 1024, D = Dy = 4 and 8; the report goes to profiles/switching_lookahead_gibbs.txt)"""
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
    u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
    y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
    nexts = [torch.randint(0, M, (B, 1), generator=gen, device=dev, dtype=torch.int32) for _ in range(3)]
    info = None
    for regime_next in nexts[:2]:      # two steps from the zeros: a full-rank Om, as most steps of a sweep see
        om, lam, c, F = k.switching_information_step(ops, regime_next, info, y)
        info = (om, lam, c)
    om, lam, c, F = k.switching_information_step(ops, nexts[2], info, y)
    pinned_regime, F1, lam1 = nexts[2][:, 0].contiguous(), F[:, 0].contiguous(), lam[:, 0].contiguous()
    step = lambda fused, factor=F1, lam=lam1: k.switching_lookahead_conditional_ancestor_index(
        ops, log_Pi, state, y, u, pinned_regime, factor, lam, fused=fused)
    one, three = step(True), step(False)
    same = bool(torch.equal(one[0], three[0]))
    bits = bool(torch.equal(one[1], three[1]) and torch.equal(one[2], three[2]))
    flags = k.read_flags(dev)
    t_fused = timed(lambda: step(True), 3, 10, 8)
    t_composed = timed(lambda: step(False), 3, 10, 8)
    t_plain = timed(lambda: step(True, None, None), 3, 10, 8)
    t_plain_composed = timed(lambda: step(False, None, None), 3, 10, 8)
    t_k32 = timed(lambda: k.switching_lookahead(ops, log_Pi, state, y), 3, 10, 8)
    t_k37 = timed(lambda: k.switching_conditional_ancestor_index(one[1], u, log_Pi, pinned_regime, F1, lam1, state), 3, 10, 8)
    regime_u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
    index = one[0].clamp(max=K - 1)
    t_k49 = timed(lambda: k.switching_kalman_conditional_draw(ops, state, index, regime_u, one[2], pinned_regime, y), 3, 10, 8)
    t_k38 = timed(lambda: k.switching_kalman_conditional_step(ops, state, index, regime_u, pinned_regime, y), 3, 10, 8)
    flags |= k.read_flags(dev)
    lines.append("B={} K={} M={} D={} Dy={} (flags {}; K48 and the composition give the same indices: {}; the same bits of "
                 "log_weight and cdf: {})".format(B, K, M, D, Dy, flags, same, bits))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("K48, one launch", *t_fused))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us   K48 takes {:.2f} of it".format(
        "K32 + K37 + K37 on zeros + torch.where", *t_composed, t_fused[0] / t_composed[0]))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("  of which K32", *t_k32))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us".format("  of which K37 with ancestor sampling", *t_k37))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us   K32 + K37: {:.1f} ({:.1f} .. {:.1f}) us".format(
        "K48 without ancestor sampling", *t_plain, *t_plain_composed))
    lines.append("  {:<52} {:9.1f} ({:.1f} .. {:.1f}) us   K38: {:.1f} ({:.1f} .. {:.1f}) us".format(
        "K49 conditional draw", *t_k49, *t_k38))
    torch.cuda.empty_cache()


def sticky(T, B):
    ops, series = contract.sticky_example(T=T, seed=0)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(dev)
    return model, [torch.from_numpy(np.broadcast_to(y, (B, y.shape[0])).copy()).to(dev) for y in series]


def abrupt(T, B):
    """Two regimes whose emissions lie 2 apart with an observation noise of 0.5 beside a state of standard deviation 0.46, a
    sticky chain: one simulated series with abrupt changes.  One observation tells the regimes apart most of the time, so a
    change shows in the step where it happens, and the regime posterior is still not a point mass around the changes (the
    report prints its spread)."""
    ops = contract.operands([0.5, 0.5], [[0.95, 0.05], [0.05, 0.95]], [0.0], [1.0], [[[0.9]], [[0.9]]], [[0.0], [0.0]],
                            [[0.2], [0.2]], [[[1.0]], [[1.0]]], [[-1.0], [1.0]], [[0.5], [0.5]])
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(dev)
    series = model.simulate(T, 1, seed=7)
    return model, [y.expand(B, y.size(1)).contiguous() for y in series]


def sweeps(lines, B=1024, K=64, T=100):
    model, ys = sticky(T, B)
    reference = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(T)]
    torch.manual_seed(3)
    for ancestor_sampling in (True, False):
        for look in (True, False):
            t = timed(lambda: rao_blackwell.conditional_switching_filter(ys, model, K, reference, lookahead=look,
                                                                         ancestor_sampling=ancestor_sampling), 1, 5, 1)
            lines.append("one sweep of conditional_switching_filter, contract.sticky_example (M=3, D=Dy=1), T={}, B={}, K={}, "
                         "ancestor_sampling={}, lookahead={}: {:.1f} ({:.1f} .. {:.1f}) us, host included".format(
                             T, B, K, ancestor_sampling, look, *t))


def autocorrelation_time(chain):
    """chain [S, T, B] of 0 / 1: the integrated autocorrelation time 1 + 2 sum_k rho_k of the indicator along the sweeps, with
    the autocovariances pooled over chains and time points (each centred by its time point's mean over chains and sweeps)
    and the sum cut at the first lag whose pooled autocorrelation is below 0.05 (or at S / 3)."""
    x = chain - chain.mean(dim=(0, 2), keepdim=True)
    S = x.size(0)
    variance = float((x * x).mean())
    if variance == 0.0:
        return float("nan")
    total = 1.0
    for lag in range(1, S // 3):
        rho = float((x[:-lag] * x[lag:]).mean()) / variance
        if rho < 0.05:
            break
        total += 2.0 * rho
    return total


def mixing(lines, name, model, ys, B, num_sweeps=60, marks=(1, 2, 5, 10, 20)):
    """Both samplers from the SAME start — every chain at regime 0 everywhere — against reference marginals p(s_t | y) from the
    look-ahead smoother with 512 particles and 512 trajectories in 16 rows (8192 trajectories).  Per sampler: the mean over
    (t, regime) of |frequency over the 1024 chains - reference| after 1, 2, 5, 10, 20 sweeps (how fast the start is
    forgotten; the floor is the sampling error of 1024 chains); then, over the second half of the sweeps: the same error of
    the frequencies pooled over those sweeps, the share of time points and of paths a sweep changes, and the integrated
    autocorrelation time of each regime's indicator."""
    T, M = len(ys), model.num_regimes
    torch.manual_seed(4)
    np.random.seed(4)
    smoothed, _ = rao_blackwell.switching_smooth([y[:16].contiguous() for y in ys], model, 512, num_trajectories=512,
                                                 lookahead=True)
    reference = smoothed["smoothed_regime_probabilities"].mean(dim=1)      # [T, M]
    top = reference.max(dim=1).values
    floor = float(torch.sqrt(reference * (1.0 - reference) / B).mean()) * 0.8      # E|N(0, s^2)| = 0.8 s
    lines.append("  {}: M = {}; the reference posterior: mean over t of 1 - max_m p(s_t = m | y) = {:.3f}, {} of {} time points "
                 "with max_m p < 0.95, {} with max_m p < 0.75; sampling floor of the error below, 1024 chains: {:.4f}".format(
                     name, M, float((1.0 - top).mean()), int((top < 0.95).sum()), T, int((top < 0.75).sum()), floor))
    start = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(T)]
    for K in (8, 16):
        for look in (True, False):
            torch.manual_seed(5)
            out = rao_blackwell.switching_particle_gibbs(ys, model, K, num_sweeps, reference=start, lookahead=look)
            paths = torch.stack(out["regimes"]).permute(2, 0, 1)      # [S, T, B]
            onehot = torch.nn.functional.one_hot(paths.long(), M).double()      # [S, T, B, M]
            error = lambda frequencies: float((frequencies - reference).abs().mean())
            forgetting = " ".join("{:.4f}".format(error(onehot[s - 1].mean(dim=1))) for s in marks)
            late = paths[num_sweeps // 2:]
            pooled = error(onehot[num_sweeps // 2:].mean(dim=(0, 2)))
            changed = float((late[1:] != late[:-1]).double().mean())
            whole = float((late[1:] != late[:-1]).any(dim=1).double().mean())
            times = [autocorrelation_time((late == regime).double()) for regime in range(M)]
            lines.append("  {:<7} K={:<3} lookahead={!s:<5} error after {} sweeps: {}; sweeps {}..{}: pooled error {:.4f}, time "
                         "points changed per sweep {:.4f}, paths changed per sweep {:.3f}, autocorrelation times {}".format(
                             name, K, look, "/".join(str(s) for s in marks), forgetting, num_sweeps // 2 + 1, num_sweeps, pooled,
                             changed, whole, " ".join("{:.2f}".format(t) for t in times)))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "switching_lookahead_gibbs.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or \
        [(1024, K, 4, D, D) for D in (4, 8) for K in (8, 64, 1024)]
    lines = ["tools/bench_switching_lookahead_gibbs.py on one {} ({}), float64 throughout, float32 observations, HIP events, "
             "warm; us per call through the provider (allocation and launch latency included): median (min .. max)".format(
                 torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for shape in shapes:
        kernels(lines, *shape)
    sweeps(lines)
    lines.append("what the look-ahead buys: T = 100, 1024 chains of 60 sweeps with ancestor sampling, both samplers from the same "
                 "start (regime 0 everywhere), errors against the look-ahead smoother's marginals (8192 trajectories)")
    mixing(lines, "sticky", *sticky(100, 1024), 1024)
    mixing(lines, "abrupt", *abrupt(100, 1024), 1024)
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
