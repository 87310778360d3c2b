"""K32 (aesmc_switching_lookahead) and K33 (aesmc_switching_kalman_draw) alone, beside K31 (aesmc_switching_kalman_step) on
the same operands in the same run: timed warm between HIP events, the median per call with the spread, the bytes each
launch moves and the fraction of the HBM peak they make.  Then, on the model of the variance test
(`contract.sticky_example`: sticky regimes, well-separated emissions), the sample variance of log Z-hat over the batch rows
of one call for the look-ahead filter and for the bootstrap on the regimes — at equal K, and with the bootstrap given the
smallest K (a power-of-two multiple) at which its pass takes at least the look-ahead's device time.
    python tools/bench_switching_lookahead.py [--out FILE] [B,K,M,D,Dy ...]
(default: 1024,4096,4,4,4 and 1024,4096,4,8,8; the report goes to profiles/switching_lookahead.txt)"""
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
PEAK_HBM = 8000e9      # MI355X, bytes/s
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
    TD = D * (D + 1) // 2
    model = contract.example_model(M, D, Dy, seed=1)
    ops = {name: torch.from_numpy(np.array(value)).to(dev) for name, value in model.items()}
    log_Pi = torch.log(ops["Pi"])
    gen = torch.Generator(device=dev).manual_seed(1)
    regime = torch.randint(0, M, (B, K), generator=gen, device=dev, dtype=torch.int32)
    mean = torch.randn(B, K, D, generator=gen, device=dev, dtype=torch.float64)
    factor = torch.randn(B, K, D, D, generator=gen, device=dev, dtype=torch.float64)
    full = factor @ factor.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64)
    rows, cols = torch.tril_indices(D, D, device=dev)
    packed = full[..., rows, cols].contiguous()
    del factor, full
    idx = torch.sort(torch.randint(0, K, (B, K), generator=gen, device=dev), dim=1).values      # as a resampler's
    u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
    y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
    state = (regime, mean, packed)
    log_w, cdf = k.switching_lookahead(ops, log_Pi, state, y)
    drawn = k.switching_kalman_draw(ops, state, idx, u, cdf, y)
    flags = k.read_flags(dev)
    finite = bool(torch.isfinite(log_w).all()) and bool(torch.isfinite(drawn[1]).all())
    del drawn
    t_look = timed(lambda: k.switching_lookahead(ops, log_Pi, state, y), 3, 10, 8)
    t_draw = timed(lambda: k.switching_kalman_draw(ops, state, idx, u, cdf, y), 3, 10, 8)
    t_step = timed(lambda: k.switching_kalman_step(ops, state, idx, u, y), 3, 10, 8)
    state_bytes = 4 + 8 * D + 8 * TD
    b_look = B * K * (state_bytes + 8 + 8 * M) + B * Dy * 4
    b_draw = B * K * (8 + 8 + 8 * M + 2 * state_bytes + 8) + B * Dy * 4
    b_step = B * K * (8 + 8 + 2 * state_bytes + 8) + B * Dy * 4
    lines.append("B={} K={} M={} D={} Dy={} (sorted ancestors; flags {}; outputs finite: {})".format(B, K, M, D, Dy, flags, finite))
    for name, t, nbytes in (("K32 look-ahead", t_look, b_look), ("K33 draw", t_draw, b_draw), ("K31 step", t_step, b_step)):
        lines.append("  {:<16} {:10.1f} ({:.1f} .. {:.1f}) us   {:8.1f} MB, {:.3f} of the peak".format(
            name, *t, nbytes / 1e6, nbytes / (t[0] * 1e-6) / PEAK_HBM))
    lines.append("  K33 / K31 = {:.3f}; a look-ahead step (K32 + K33) / a bootstrap step (K31) = {:.2f}".format(
        t_draw[0] / t_step[0], (t_look[0] + t_draw[0]) / t_step[0]))
    del regime, mean, packed, idx, u, log_w, cdf
    torch.cuda.empty_cache()


def variances(lines, R=1024, K=256, T=12):
    ops, series = contract.sticky_example(T=T, seed=0)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(dev)
    ys = [torch.from_numpy(np.broadcast_to(y, (R, y.shape[0])).copy()).to(dev) for y in series]

    def run(filter_fn, particles):
        torch.manual_seed(11)
        np.random.seed(11)
        log_z = filter_fn(ys, model, particles, resampling="systematic")["log_marginal_likelihood"]
        t = timed(lambda: filter_fn(ys, model, particles, resampling="systematic"), 1, 5, 1)
        return float(log_z.var(unbiased=True)), float(log_z.mean()), t

    lines.append("contract.sticky_example (M=3, D=Dy=1, T={}), {} replicas as the batch rows of one call, systematic resampling: "
                 "variance and mean of log Z-hat, device time of the whole pass".format(T, R))
    var_a, mean_a, t_a = run(rao_blackwell.adapted_switching_filter, K)
    lines.append("  look-ahead  K={:<6} variance {:.3e}  mean {:.6f}  {:9.1f} ({:.1f} .. {:.1f}) us".format(K, var_a, mean_a, *t_a))
    particles = K
    while True:
        var_b, mean_b, t_b = run(rao_blackwell.switching_filter, particles)
        lines.append("  bootstrap   K={:<6} variance {:.3e}  mean {:.6f}  {:9.1f} ({:.1f} .. {:.1f}) us{}".format(
            particles, var_b, mean_b, *t_b, "   (equal K: variance ratio {:.1f})".format(var_b / var_a) if particles == K else ""))
        if t_b[0] >= t_a[0] or particles >= 64 * K:
            break
        particles *= 2
    lines.append("  at equal device time (bootstrap K={}, {:.2f} of the look-ahead's time or more): variance ratio {:.1f}".format(
        particles, t_b[0] / t_a[0], var_b / var_a))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "switching_lookahead.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or [(1024, 4096, 4, 4, 4), (1024, 4096, 4, 8, 8)]
    lines = ["tools/bench_switching_lookahead.py on one {} ({}), float64 state, float32 observations, HIP events, warm; us per "
             "call: median (min .. max); bytes the launch moves; fraction of the {:.0f} GB/s HBM peak".format(
                 torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode(), PEAK_HBM / 1e9)]
    for shape in shapes:
        kernels(lines, *shape)
    variances(lines)
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
