"""Monte Carlo EM for a switching linear-Gaussian state-space model, every parameter learned: examples/slds_em.py's loop with
the library's E-step reduction and M-step.

    python examples/slds_em_full.py [--dim 2] [--particles 128] [--trajectories 128] [--batch 16] [--timesteps 100]
                                    [--iterations 10] [--seed 0]

Simulates series from a two-regime model, starts from a perturbed copy of ALL ten parameters (pi0, Pi, m0, s0, A, b, q, C, d,
r) and iterates

    E-step   `aesmc_amd.rao_blackwell.switching_smooth_states` with return_trajectories (K32, K33; K34, K35; K31 forced, K34,
             K36), then `switching_expected_statistics`: one K45 launch per timestep sums the trajectories' moments into the
             expected sufficient statistics per regime — no [T, B, N, D, D] stack, no loop over regimes, no atomics;
    M-step   `switching_m_step`: closed form on the statistics, a new model

and prints, per iteration, the look-ahead filter's evidence estimate per step and the distance of A and C from the truth.
The E-step is Monte Carlo (only the regimes are sampled), so the estimate need not rise monotonically; C and d are
identified only up to the usual change of basis of the latent, which is why the evidence is the figure to watch.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import aesmc_amd as aesmc  # noqa: F401
from aesmc_amd import rao_blackwell
from slds_em import build, true_parameters


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
    exact = build(truth, device)
    observations = exact.simulate(args.timesteps, args.batch, seed=args.seed + 1)
    rng = np.random.default_rng(args.seed + 2)
    noisy = lambda value, scale: np.asarray(value, dtype=np.float64) + scale * rng.standard_normal(np.shape(value))
    model = build(dict(pi0=np.array([0.6, 0.4]), Pi=np.array([[0.7, 0.3], [0.3, 0.7]]), m0=noisy(truth["m0"], 0.3), s0=1.5,
                       A=noisy(truth["A"], 0.15), b=noisy(truth["b"], 0.3), q=np.full((1, D), 0.5), C=noisy(truth["C"], 0.1),
                       d=noisy(truth["d"], 0.1), r=np.full((1, D), 0.5)), device)
    for iteration in range(args.iterations + 1):
        out, log_z = rao_blackwell.switching_smooth_states(observations, model, args.particles,
                                                           num_trajectories=args.trajectories, lookahead=True,
                                                           return_trajectories=True)
        print("iteration {:2d}: log Z-hat per step {:9.5f}   |A - A_true| {:.4f}   |C - C_true| {:.4f}   q {:.3f}   r {:.3f}   "
              "Pi diagonal {}".format(iteration, log_z.mean().item() / args.timesteps, (model.A - exact.A).norm().item(),
                                      (model.C - exact.C).norm().item(), model.q.mean().item(), model.r.mean().item(),
                                      ", ".join("{:.3f}".format(v) for v in model.Pi.diagonal().tolist())))
        if iteration == args.iterations:
            break
        statistics = rao_blackwell.switching_expected_statistics(out, observations, model)
        model = rao_blackwell.switching_m_step(statistics, model)
    reference = rao_blackwell.adapted_switching_filter(observations, exact, args.particles)["log_marginal_likelihood"]
    print("at the true parameters: log Z-hat per step {:9.5f}".format(reference.mean().item() / args.timesteps))


if __name__ == "__main__":
    main()
