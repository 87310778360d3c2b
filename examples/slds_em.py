"""Monte Carlo EM for a switching linear-Gaussian state-space model: the switching counterpart of examples/lgssm_em.py.

    python examples/slds_em.py [--dim 2] [--particles 128] [--trajectories 128] [--batch 16] [--timesteps 100]
                               [--iterations 10] [--seed 0]

Simulates series from a two-regime model, starts from perturbed Pi, A and b, and iterates

    E-step   `aesmc_amd.rao_blackwell.switching_smooth_states` with return_trajectories: the look-ahead filter (K32, K33),
             regime trajectories by Rao-Blackwellised backward simulation (K34, K35), and along every trajectory the exact
             smoothed moments of the continuous state with the lag-one cross-covariance (K31 forced, K34, K36);
    M-step   in plain torch.  Pi from the trajectories' transition counts; A[j] and b[j] from the regression of z_{t+1} on
             (z_t, 1) over the steps whose s_{t+1} = j, with the expected sufficient statistics E[z_{t+1} z_t^T],
             E[z_t z_t^T], E[z_{t+1}], E[z_t].  q, C, d, r, pi0, m0, s0 are held at their true values.

and prints, per iteration, the look-ahead filter's evidence estimate per step and the distance of A from the truth.  The
E-step is Monte Carlo (only the regimes are sampled), so the estimate need not rise monotonically.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import aesmc_amd as aesmc  # noqa: F401
from aesmc_amd import rao_blackwell


def true_parameters(D, seed):
    """Two sticky regimes: a slow rotation that keeps the state and a fast one that shrinks it, with different offsets."""
    rng = np.random.default_rng(seed)
    Pi = np.array([[0.95, 0.05], [0.10, 0.90]])
    A = np.stack([np.linalg.qr(rng.standard_normal((D, D)))[0] * scale for scale in (0.95, 0.5)])
    b = np.stack([np.zeros(D), np.full(D, 1.0)])
    return {"pi0": np.full(2, 0.5), "Pi": Pi, "m0": np.zeros(D), "s0": 1.0, "A": A, "b": b, "q": np.full((1, D), 0.3),
            "C": np.eye(D)[None], "d": np.zeros((1, D)), "r": np.full((1, D), 0.3)}


def build(parameters, device):
    keys = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
    return rao_blackwell.SwitchingLinearGaussian(*[parameters[key] for key in keys]).to(device)


def m_step(out, M, D, previous):
    """(Pi [M,M], A [M,D,D], b [M,D]) from the E-step's trajectories, as float64 tensors on their device.  `previous`: the
    model of the E-step — a regime no trajectory leaves keeps its row of Pi, one none enters keeps its A[j] and b[j]."""
    regimes = torch.stack(out["regimes"]).long()                                            # [T,B,N]
    means = torch.stack(out["means"])                                                       # [T,B,N,D]
    second = rao_blackwell.unpack_covariance(torch.stack(out["covariances"]), D) + means.unsqueeze(-1) * means.unsqueeze(-2)
    lagged = torch.stack(out["cross_covariances"]) + means[1:].unsqueeze(-1) * means[:-1].unsqueeze(-2)   # E[z_{t+1} z_t^T]
    counts = torch.zeros(M, M, dtype=torch.float64, device=means.device)
    counts.index_put_((regimes[:-1].reshape(-1), regimes[1:].reshape(-1)),
                      torch.ones(regimes[1:].numel(), dtype=torch.float64, device=means.device), accumulate=True)
    left = counts.sum(dim=1, keepdim=True)
    Pi = torch.where(left > 0, counts / left.clamp(min=1.0), previous.Pi)
    A, b = [], []
    for j in range(M):
        w = (regimes[1:] == j).to(torch.float64)                                            # [T-1,B,N]
        if not bool(w.any()):
            A.append(previous.A[j]), b.append(previous.b[j])
            continue
        total = lambda x: (w.reshape(w.shape + (1,) * (x.dim() - 3)) * x).sum(dim=(0, 1, 2))
        Sxx, Sx, Syx, Sy, n = total(second[:-1]), total(means[:-1]), total(lagged), total(means[1:]), w.sum()
        # [A b] [[Sxx, Sx], [Sx^T, n]] = [Syx, Sy]
        gram = torch.cat([torch.cat([Sxx, Sx[:, None]], dim=1), torch.cat([Sx[None, :], n.reshape(1, 1)], dim=1)], dim=0)
        solved = torch.linalg.solve(gram, torch.cat([Syx, Sy[:, None]], dim=1).t()).t()     # [D, D+1]
        A.append(solved[:, :D]), b.append(solved[:, D])
    return Pi, torch.stack(A), torch.stack(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--particles", type=int, default=128)
    ap.add_argument("--trajectories", type=int, default=128)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.timesteps < 2:
        ap.error("--timesteps must be at least 2: the M-step needs a transition")

    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    D, M = args.dim, 2
    truth = true_parameters(D, args.seed)
    observations = build(truth, device).simulate(args.timesteps, args.batch, seed=args.seed + 1)
    rng = np.random.default_rng(args.seed + 2)
    current = dict(truth, Pi=np.array([[0.7, 0.3], [0.3, 0.7]]), A=truth["A"] + 0.15 * rng.standard_normal((M, D, D)),
                   b=truth["b"] + 0.3 * rng.standard_normal((M, D)))
    A_true = torch.from_numpy(truth["A"]).to(device)
    for iteration in range(args.iterations + 1):
        model = build(current, device)
        out, log_z = rao_blackwell.switching_smooth_states(observations, model, args.particles,
                                                           num_trajectories=args.trajectories, lookahead=True,
                                                           return_trajectories=True)
        print("iteration {:2d}: log Z-hat per step {:9.5f}   |A - A_true| {:.4f}   Pi diagonal {}".format(
            iteration, log_z.mean().item() / args.timesteps, (model.A - A_true).norm().item(),
            ", ".join("{:.3f}".format(v) for v in model.Pi.diagonal().tolist())))
        if iteration == args.iterations:
            break
        Pi, A, b = m_step(out, M, D, model)
        current = dict(current, Pi=Pi.cpu().numpy(), A=A.cpu().numpy(), b=b.cpu().numpy())
    exact = build(truth, device)
    reference = rao_blackwell.adapted_switching_filter(observations, exact, args.particles)["log_marginal_likelihood"]
    print("at the true parameters: log Z-hat per step {:9.5f}".format(reference.mean().item() / args.timesteps))


if __name__ == "__main__":
    main()
