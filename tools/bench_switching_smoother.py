"""K34 (aesmc_switching_information_step) and K35 (aesmc_switching_backward_scores) alone, beside K21's draw on the scores
(rows [B N, K], one trajectory each), K36 (aesmc_switching_smooth_combine, the state smoother's launch per timestep, over the
same B N trajectories as K34) without and with the cross-covariance and, in the same run, the batched `torch.linalg` composition of the same scores: timed
warm between HIP events, the median per call with the spread.  Then, on `contract.sticky_example` (sticky regimes,
well-separated emissions), how often the most probable smoothed regime is the true one beside the filtered one, and the
device time of the whole backward pass beside the filter's.
    python tools/bench_switching_smoother.py [--out FILE] [B,K,N,M,D,Dy ...]
(default: 64,1024,64,4,4,4 and 64,1024,64,4,8,8; the report goes to profiles/switching_smoother.txt)"""
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


def composed_scores(log_Pi, regime_next, factor, lam, state, log_w, D):
    """The same scores by batched torch.linalg on full matrices: one Cholesky factor and one triangular solve per pair."""
    regime, mean, cov = state
    F = torch.tril(rao_blackwell.unpack_covariance(factor, D))               # [B,N,D,D], Om = F F^T
    P = rao_blackwell.unpack_covariance(cov, D)                              # [B,K,D,D]
    Ft = F.transpose(-1, -2)
    t = torch.einsum("bnij,bkj->bnki", Ft, mean)                             # Phi m
    h = lam.unsqueeze(2) - torch.einsum("bnij,bnkj->bnki", F, t)             # lam - Om m
    W = torch.einsum("bnij,bkjl->bnkil", Ft, P)                              # Phi P
    v = torch.einsum("bnkil,bnkl->bnki", W, h)
    Lam = torch.einsum("bnkil,bnlj->bnkij", W, F) + torch.eye(D, dtype=torch.float64, device=F.device)
    G = torch.linalg.cholesky(Lam)
    x = torch.linalg.solve_triangular(G, v.unsqueeze(-1), upper=False).squeeze(-1)
    hph = torch.einsum("bnki,bkij,bnkj->bnk", h, P, h)
    prior = log_Pi[regime.long().unsqueeze(1), regime_next.long().unsqueeze(2)]
    return log_w.unsqueeze(1) + prior + torch.einsum("bni,bki->bnk", lam, mean) - 0.5 * t.pow(2).sum(-1) + \
        0.5 * (hph - x.pow(2).sum(-1)) - torch.log(torch.diagonal(G, dim1=-2, dim2=-1)).sum(-1)


def kernels(lines, B, K, N, M, D, Dy):
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
    state = (regime, mean, full[..., rows, cols].contiguous())
    del factor, full
    log_w = torch.randn(B, K, generator=gen, device=dev, dtype=torch.float64)
    u = torch.rand(B * N, 1, generator=gen, device=dev, dtype=torch.float64)
    y = torch.randn(B, Dy, generator=gen, device=dev, dtype=torch.float32)
    nexts = [torch.randint(0, M, (B, N), generator=gen, device=dev, dtype=torch.int32) for _ in range(3)]
    info = None
    for regime_next in nexts[:2]:      # two steps from the zeros: a full-rank Om, as most steps of a pass see
        om, lam, c, F = k.switching_information_step(ops, regime_next, info, y)
        info = (om, lam, c)
    regime_next = nexts[2]
    om, lam, c, F = k.switching_information_step(ops, regime_next, info, y)
    scores = k.switching_backward_scores(log_Pi, regime_next, F, lam, state, log_w)
    composed = composed_scores(log_Pi, regime_next, F, lam, state, log_w, D)
    difference = float((scores - composed).abs().max())
    flags = k.read_flags(dev)
    t_info = timed(lambda: k.switching_information_step(ops, regime_next, info, y), 3, 10, 8)
    root = torch.randn(2, B, N, D, D, generator=gen, device=dev, dtype=torch.float64)
    packed = (root @ root.transpose(-1, -2) / D + 0.1 * torch.eye(D, device=dev, dtype=torch.float64))[..., rows, cols]
    moments, cov_next = (torch.randn(B, N, D, generator=gen, device=dev, dtype=torch.float64), packed[0].contiguous()), \
        packed[1].contiguous()
    t_combine = timed(lambda: k.switching_smooth_combine(None, None, moments, F, lam), 3, 10, 8)
    t_cross = timed(lambda: k.switching_smooth_combine(ops, regime_next, moments, F, lam, info[0], cov_next), 3, 10, 8)
    flags |= k.read_flags(dev)
    t_score = timed(lambda: k.switching_backward_scores(log_Pi, regime_next, F, lam, state, log_w), 3, 10, 8)
    t_draw = timed(lambda: k.backward_sample(scores.reshape(B * N, K), None, None, None, u), 3, 10, 8)
    t_torch = timed(lambda: composed_scores(log_Pi, regime_next, F, lam, state, log_w, D), 2, 5, 2)
    pairs = B * N * K
    lines.append("B={} K={} N={} M={} D={} Dy={} (flags {}; largest |K35 - torch.linalg| {:.2e})".format(
        B, K, N, M, D, Dy, flags, difference))
    lines.append("  {:<34} {:10.1f} ({:.1f} .. {:.1f}) us".format("K34 information step", *t_info))
    lines.append("  {:<34} {:10.1f} ({:.1f} .. {:.1f}) us   {:.1f} times K34".format(
        "K36 smoothed moments", *t_combine, t_combine[0] / t_info[0]))
    lines.append("  {:<34} {:10.1f} ({:.1f} .. {:.1f}) us   {:.1f} times K34".format(
        "K36 with the cross-covariance", *t_cross, t_cross[0] / t_info[0]))
    lines.append("  {:<34} {:10.1f} ({:.1f} .. {:.1f}) us   {:.3f} ns per pair, {:.1f} MB of scores written".format(
        "K35 pair scores", *t_score, t_score[0] * 1e3 / pairs, 8 * pairs / 1e6))
    lines.append("  {:<34} {:10.1f} ({:.1f} .. {:.1f}) us".format("K21 draw, rows [B N, K]", *t_draw))
    lines.append("  {:<34} {:10.1f} ({:.1f} .. {:.1f}) us   K35 is {:.1f} times faster".format(
        "torch.linalg composition of K35", *t_torch, t_torch[0] / t_score[0]))
    lines.append("  a backward step = K34 + K35 + K21: {:.1f} us, of which K35 {:.0%}, K21 {:.0%}".format(
        t_info[0] + t_score[0] + t_draw[0], t_score[0] / (t_info[0] + t_score[0] + t_draw[0]),
        t_draw[0] / (t_info[0] + t_score[0] + t_draw[0])))
    del scores, composed
    torch.cuda.empty_cache()


def sticky_truth(T, seed=0):
    """The regimes `contract.sticky_example(T, seed)` simulated (it returns only the series): its generator, replayed."""
    ops, series = contract.sticky_example(T=T, seed=seed)
    rng = np.random.default_rng([seed, 1999])
    truth, s, z = [], None, None
    for t in range(T):
        s = rng.choice(3, p=ops["pi0"] if t == 0 else ops["Pi"][s])
        z = ops["m0"] + ops["s0"] * rng.standard_normal(1) if t == 0 else \
            ops["A"][s] @ z + ops["b"][s] + ops["q"][s] * rng.standard_normal(1)
        y = ops["C"][s] @ z + ops["d"][s] + ops["r"][s] * rng.standard_normal(1)
        assert np.array_equal(y, series[t]), "the replay left the example's generator"
        truth.append(int(s))
    return ops, series, np.array(truth)


def accuracy(lines, R=64, K=256, N=256, T=200):
    ops, series, truth = sticky_truth(T)
    model = rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(dev)
    ys = [torch.from_numpy(np.broadcast_to(y, (R, y.shape[0])).copy()).to(dev) for y in series]
    truth = torch.from_numpy(truth).to(dev)[:, None]
    lines.append("contract.sticky_example (M=3, D=Dy=1, T={}), {} replicas as the batch rows of one call, K={}, N={}: how often "
                 "the most probable regime is the true one, and the device time of the pass".format(T, R, K, N))
    for name, run in (("bootstrap", rao_blackwell.switching_filter), ("look-ahead", rao_blackwell.adapted_switching_filter)):
        torch.manual_seed(11)
        np.random.seed(11)
        filtered = run(ys, model, K, resampling="systematic", return_moments=True)
        smoothed = rao_blackwell.switching_backward_simulate(filtered, model, ys, num_trajectories=N)
        hit_f = (filtered["regime_probabilities"].argmax(dim=-1) == truth).double().mean().item()
        hit_s = (smoothed["smoothed_regime_probabilities"].argmax(dim=-1) == truth).double().mean().item()
        t_f = timed(lambda: run(ys, model, K, resampling="systematic"), 1, 5, 1)
        t_s = timed(lambda: rao_blackwell.switching_backward_simulate(filtered, model, ys, num_trajectories=N), 1, 5, 1)
        lines.append("  {:<11} filtered {:.4f}  smoothed {:.4f}   filter {:9.1f} ({:.1f} .. {:.1f}) us   backward pass {:9.1f} "
                     "({:.1f} .. {:.1f}) us".format(name, hit_f, hit_s, *t_f, *t_s))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "switching_smoother.txt")
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    shapes = [tuple(int(x) for x in arg.split(",")) for arg in argv] or [(64, 1024, 64, 4, 4, 4), (64, 1024, 64, 4, 8, 8)]
    lines = ["tools/bench_switching_smoother.py on one {} ({}), float64 throughout, float32 observations, HIP events, warm; us "
             "per call: median (min .. max)".format(torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode())]
    for shape in shapes:
        kernels(lines, *shape)
    accuracy(lines)
    report = "\n".join(lines) + "\n"
    print(report, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write(report)


if __name__ == "__main__":
    main(sys.argv[1:])
