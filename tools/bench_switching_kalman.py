"""K31 (aesmc_switching_kalman_step: one step of the Rao-Blackwellised filter of a switching linear-Gaussian model) alone,
beside the same step written as batched torch.linalg calls on the same device in the same run — gathers, two batched
products for the predict, torch.linalg.cholesky, two torch.linalg.solve_triangular and the downdate over [B K, D, D]
temporaries (on FULL covariances, which spares the composition the packing), and the factorisation and the two solves of
that composition once more alone: they are what its time consists of.  Everything is timed warm between HIP events;
the median per call is reported with the spread, K31 beside the bytes its launch moves and the fraction of the HBM peak
they make.
    python tools/bench_switching_kalman.py [--out FILE] [B,K,M,D,Dy ...]
(default: 1024,4096,4,4,4 and 1024,4096,4,8,8; the report goes to profiles/switching_kalman.txt)
    python tools/bench_switching_kalman.py --missing [--parent-report FILE] [--out FILE] [B,K,M,D,Dy ...]
the masked step K39 (aesmc_switching_kalman_masked_step) beside K31 on the same inputs in the same run: under a mask that
observes everything (K39 then computes what K31 does), one drawn with p = 0.6 per component, and one that observes nothing
(the prediction).  --parent-report: a report this tool wrote on the commit before K39 in the same session, whose K31 lines
are quoted beside.  A measurement, no threshold; the report goes to profiles/switching_missing.txt.
    python tools/bench_switching_kalman.py --discrete [--out FILE] [B,K,M,D,Dy ...]
a step of the discrete particle filter (K43 aesmc_switching_lookahead_scores + K44 aesmc_switching_optimal_resample + K31
forced through the parents) beside a step of the fully adapted filter (K32 + K2 + K33) on the same stored system in the same
run, each launch alone and the three together (default: 1024,1024,4,4,4 and 1024,1024,4,8,8).  A measurement, no
threshold; the report goes to profiles/discrete_filter.txt."""
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
HALF_LOG_2PI = 0.9189385332046727


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


def predict_and_innovate(ops, regime, mean, full_cov, idx, u, y):
    """(regime, predicted mean, predicted covariance, e, U = C P-, S) from gathers and batched products."""
    M, D = ops["A"].size(0), ops["A"].size(2)
    previous = torch.gather(regime, 1, idx).long()
    m = torch.gather(mean, 1, idx.unsqueeze(-1).expand(-1, -1, D))
    P = torch.gather(full_cov, 1, idx[:, :, None, None].expand(-1, -1, D, D))
    s = (ops["cdf"][previous][..., :M - 1] <= u.unsqueeze(-1)).sum(dim=-1)
    A, C = ops["A"][s], ops["C"][s]
    predicted_mean = (A @ m.unsqueeze(-1)).squeeze(-1) + ops["b"][s]
    predicted = A @ P @ A.transpose(-1, -2) + torch.diag_embed(ops["q"][s] ** 2)
    e = y.to(torch.float64).unsqueeze(1) - (C @ predicted_mean.unsqueeze(-1)).squeeze(-1) - ops["d"][s]
    U = C @ predicted
    S = U @ C.transpose(-1, -2) + torch.diag_embed(ops["r"][s] ** 2)
    return s, predicted_mean, predicted, e, U, S


def factor_and_solve(S, e, U):
    """(Lam, v, V): torch.linalg.cholesky and the two torch.linalg.solve_triangular over the [B K] small systems."""
    lam = torch.linalg.cholesky(S)
    return (lam, torch.linalg.solve_triangular(lam, e.unsqueeze(-1), upper=False),
            torch.linalg.solve_triangular(lam, U, upper=False))


def composition(ops, regime, mean, full_cov, idx, u, y):
    """The step from batched torch operations: (regime int32, mean, FULL covariance, log-weight)."""
    Dy = ops["C"].size(1)
    s, predicted_mean, predicted, e, U, S = predict_and_innovate(ops, regime, mean, full_cov, idx, u, y)
    lam, v, V = factor_and_solve(S, e, U)
    log_w = -0.5 * (v * v).sum(dim=(-2, -1)) - torch.log(torch.diagonal(lam, dim1=-2, dim2=-1)).sum(dim=-1) - Dy * HALF_LOG_2PI
    return (s.to(torch.int32), predicted_mean + (V.transpose(-1, -2) @ v).squeeze(-1), predicted - V.transpose(-1, -2) @ V,
            log_w)


def missing_leg(shapes, parent_report):
    """The report of --missing: K31 and K39 under three masks, per shape."""
    lines = ["tools/bench_switching_kalman.py --missing on one {} ({}), float64 state, float32 observations, HIP events, warm; "
             "us per call: median (min .. max)".format(torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for B, K, M, D, Dy in shapes:
        model = contract.example_model(M, D, Dy, seed=1)
        ops = {name: torch.from_numpy(np.array(value)).to(dev) for name, value in model.items()}
        gen = torch.Generator(device=dev).manual_seed(1)
        regime = torch.randint(0, M, (B, K), generator=gen, device=dev, dtype=torch.int32)
        mean = torch.randn(B, K, D, generator=gen, device=dev, dtype=torch.float64)
        factor = torch.randn(B, K, D, D, generator=gen, device=dev, dtype=torch.float64)
        full = factor @ factor.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64)
        rows, cols = torch.tril_indices(D, D, device=dev)
        packed = (0.5 * (full + full.transpose(-1, -2)))[..., rows, cols].contiguous()
        del factor, full
        idx = torch.sort(torch.randint(0, K, (B, K), generator=gen, device=dev), dim=1).values      # as a resampler's
        u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
        y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
        masks = (("everything observed", torch.ones((B, Dy), dtype=torch.bool, device=dev)),
                 ("p = 0.6 per component", torch.rand(B, Dy, generator=gen, device=dev) < 0.6),
                 ("nothing observed", torch.zeros((B, Dy), dtype=torch.bool, device=dev)))
        plain = k.switching_kalman_step(ops, (regime, mean, packed), idx, u, y)
        same = all(torch.equal(a, b) for a, b in zip(plain, k.switching_kalman_step(ops, (regime, mean, packed), idx, u, y,
                                                                                    observed=masks[0][1])))
        lines.append("B={} K={} M={} D={} Dy={} (sorted ancestors; flags {}; K39 with everything observed equals K31 bit for "
                     "bit: {})".format(B, K, M, D, Dy, k.read_flags(dev), same))
        del plain
        lines.append("  K31                                   {:10.1f} ({:.1f} .. {:.1f}) us".format(
            *timed(lambda: k.switching_kalman_step(ops, (regime, mean, packed), idx, u, y), 3, 10, 8)))
        for name, mask in masks:
            lines.append("  K39, {:<32s} {:10.1f} ({:.1f} .. {:.1f}) us".format(name, *timed(
                lambda: k.switching_kalman_step(ops, (regime, mean, packed), idx, u, y, observed=mask), 3, 10, 8)))
        del packed, regime, mean, idx, u
        torch.cuda.empty_cache()
    if parent_report is not None:
        lines.append("K31 on the commit before K39, this tool's own report from the same session:")
        with open(parent_report) as handle:
            lines += ["  " + line.rstrip() for line in handle if line.startswith("B=") or line.startswith("  K31")]
    return lines


def discrete_leg(shapes):
    """The report of --discrete: the launches of a discrete step and of an adapted step, alone and together, per shape."""
    from aesmc_amd import _ops
    lines = ["tools/bench_switching_kalman.py --discrete on one {} ({}), float64 state, float32 observations, HIP events, warm; "
             "us per call: median (min .. max)".format(torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for B, K, M, D, Dy in shapes:
        model = contract.example_model(M, D, Dy, seed=1)
        ops = {name: torch.from_numpy(np.array(value)).to(dev) for name, value in model.items()}
        edges = (torch.arange(M, dtype=torch.float64, device=dev) + 1.0) / M
        forced = dict(ops, cdf0=edges, cdf=edges.expand(M, M).contiguous())
        log_Pi = torch.log(ops["Pi"])
        gen = torch.Generator(device=dev).manual_seed(1)
        regime = torch.randint(0, M, (B, K), generator=gen, device=dev, dtype=torch.int32)
        mean = torch.randn(B, K, D, generator=gen, device=dev, dtype=torch.float64)
        factor = torch.randn(B, K, D, D, generator=gen, device=dev, dtype=torch.float64)
        full = factor @ factor.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64)
        rows, cols = torch.tril_indices(D, D, device=dev)
        packed = (0.5 * (full + full.transpose(-1, -2)))[..., rows, cols].contiguous()
        del factor, full
        state = (regime, mean, packed)
        stored = torch.log_softmax(torch.randn(B, K, generator=gen, device=dev, dtype=torch.float64), dim=1)
        row_u = torch.rand(B, generator=gen, device=dev, dtype=torch.float64)
        u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
        y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
        scores, _ = k.switching_lookahead_scores(ops, log_Pi, state, y)
        parent, chosen, _, _, count = k.switching_optimal_resample(stored, scores, row_u, K)
        forced_u = (chosen.to(torch.float64) + 0.5) / M
        log_w, cdf = k.switching_lookahead(ops, log_Pi, state, y)
        index = _kernels.as_index(_ops.resample_step(log_w, row_u, None, want_lse=True)[0])
        kept = int((torch.sort(parent, dim=1).values.diff(dim=1) != 0).sum().item()) + B
        lines.append("B={} K={} M={} D={} Dy={} ({} candidates per row; flags {}; live slots {}; distinct parents per row: "
                     "discrete {:.0f}, adapted {:.0f})".format(
                         B, K, M, D, Dy, K * M, k.read_flags(dev), int(count.min().item()), kept / B,
                         (int((index.diff(dim=1) != 0).sum().item()) + B) / B))

        def discrete_step():
            s, _ = k.switching_lookahead_scores(ops, log_Pi, state, y)
            p, c, _, _, _ = k.switching_optimal_resample(stored, s, row_u, K)
            return k.switching_kalman_step(forced, state, p, (c.to(torch.float64) + 0.5) / M, y)

        def adapted_step():
            w, rows_ = k.switching_lookahead(ops, log_Pi, state, y)
            i = _kernels.as_index(_ops.resample_step(w, row_u, None, want_lse=True)[0])
            return k.switching_kalman_draw(ops, state, i, u, rows_, y)

        legs = (("K43 scores", lambda: k.switching_lookahead_scores(ops, log_Pi, state, y)),
                ("K44 optimal resampling", lambda: k.switching_optimal_resample(stored, scores, row_u, K)),
                ("K31 forced, idx = parent", lambda: k.switching_kalman_step(forced, state, parent, forced_u, y)),
                ("discrete step (K43 + K44 + K31)", discrete_step),
                ("K32 look-ahead", lambda: k.switching_lookahead(ops, log_Pi, state, y)),
                ("K2 resampling", lambda: _ops.resample_step(log_w, row_u, None, want_lse=True)),
                ("K33 draw", lambda: k.switching_kalman_draw(ops, state, index, u, cdf, y)),
                ("adapted step (K32 + K2 + K33)", adapted_step))
        medians = {}
        for name, fn in legs:
            result = timed(fn, 3, 10, 8)
            medians[name] = result[0]
            lines.append("  {:<36s} {:10.1f} ({:.1f} .. {:.1f}) us".format(name, *result))
        lines.append("  discrete / adapted = {:.2f}x".format(medians[legs[3][0]] / medians[legs[7][0]]))
        del packed, regime, mean, state, scores, cdf
        torch.cuda.empty_cache()
    return lines


def main(argv):
    if "--discrete" in argv:
        argv = [arg for arg in argv if arg != "--discrete"]
        out_path = os.path.join(ROOT, "profiles", "discrete_filter.txt")
        if "--out" in argv:
            at = argv.index("--out")
            out_path = argv[at + 1]
            argv = argv[:at] + argv[at + 2:]
        shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or [(1024, 1024, 4, 4, 4), (1024, 1024, 4, 8, 8)]
        report = "\n".join(discrete_leg(shapes)) + "\n"
        print(report, end="")
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as handle:
            handle.write(report)
        return
    missing = "--missing" in argv
    argv = [arg for arg in argv if arg != "--missing"]
    parent_report = None
    if "--parent-report" in argv:
        at = argv.index("--parent-report")
        parent_report = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    out_path = os.path.join(ROOT, "profiles", "switching_missing.txt" if missing else "switching_kalman.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or [(1024, 4096, 4, 4, 4), (1024, 4096, 4, 8, 8)]
    if missing:
        report = "\n".join(missing_leg(shapes, parent_report)) + "\n"
        print(report, end="")
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as handle:
            handle.write(report)
        return
    lines = ["tools/bench_switching_kalman.py on one {} ({}), float64 state, float32 observations, HIP events, warm; us per "
             "call: median (min .. max); bytes the launch moves; fraction of the {:.0f} GB/s HBM peak".format(
                 torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode(), PEAK_HBM / 1e9)]
    for B, K, M, D, Dy in shapes:
        TD = D * (D + 1) // 2
        model = contract.example_model(M, D, Dy, seed=1)
        ops = {name: torch.from_numpy(np.array(value)).to(dev) for name, value in model.items()}
        gen = torch.Generator(device=dev).manual_seed(1)
        regime = torch.randint(0, M, (B, K), generator=gen, device=dev, dtype=torch.int32)
        mean = torch.randn(B, K, D, generator=gen, device=dev, dtype=torch.float64)
        factor = torch.randn(B, K, D, D, generator=gen, device=dev, dtype=torch.float64)
        full = factor @ factor.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64)
        full = 0.5 * (full + full.transpose(-1, -2))
        rows, cols = torch.tril_indices(D, D, device=dev)
        packed = full[..., rows, cols].contiguous()
        del factor
        idx = torch.sort(torch.randint(0, K, (B, K), generator=gen, device=dev), dim=1).values      # as a resampler's
        u = torch.rand(B, K, generator=gen, device=dev, dtype=torch.float64)
        y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
        kernel = lambda: k.switching_kalman_step(ops, (regime, mean, packed), idx, u, y)
        torch_step = lambda: composition(ops, regime, mean, full, idx, u, y)
        got, want = kernel(), torch_step()
        flags = k.read_flags(dev)
        same_regimes = bool(torch.equal(got[0], want[0]))
        differences = (float((got[1] - want[1]).abs().max()),
                       float((rao_blackwell.unpack_covariance(got[2], D) - want[2]).abs().max()),
                       float((got[3] - want[3]).abs().max()))
        del got, want
        t_kernel = timed(kernel, 3, 10, 8)
        t_torch = timed(torch_step, 1, 3, 1)
        _, _, _, e, U, S = predict_and_innovate(ops, regime, mean, full, idx, u, y)
        t_factor = timed(lambda: factor_and_solve(S, e, U), 1, 3, 1)
        del e, U, S
        nbytes = B * K * (8 + 8 + 2 * (4 + 8 * D + 8 * TD) + 8) + B * Dy * 4
        lines.append("B={} K={} M={} D={} Dy={} (sorted ancestors; flags {}; regimes equal: {}; largest difference from the "
                     "composition: mean {:.1e}, covariance {:.1e}, log-weight {:.1e})".format(
                         B, K, M, D, Dy, flags, same_regimes, *differences))
        lines.append("  K31                                   {:10.1f} ({:.1f} .. {:.1f}) us   {:8.1f} MB, {:.3f} of the peak".format(
            *t_kernel, nbytes / 1e6, nbytes / (t_kernel[0] * 1e-6) / PEAK_HBM))
        lines.append("  batched torch.linalg composition      {:10.1f} ({:.1f} .. {:.1f}) us".format(*t_torch))
        lines.append("    its cholesky + 2 solve_triangular alone {:8.1f} ({:.1f} .. {:.1f}) us: {:.0%} of the composition".format(
            *t_factor, t_factor[0] / t_torch[0]))
        lines.append("  composition / K31 = {:.1f}x (where the batched factorisation's cost per matrix makes up the composition's "
                     "time, this ratio says little about K31: its fraction of the HBM peak is the figure to judge it by)".format(
                         t_torch[0] / t_kernel[0]))
        del full, packed, regime, mean, idx, u
        torch.cuda.empty_cache()
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
