"""Gradient learning of a switching linear-Gaussian state-space model, every parameter: Adam on the collapsed-mixture
evidence, beside examples/slds_em_full.py's Monte Carlo EM on the same data.

    python examples/slds_sgd.py [--dim 2] [--batch 16] [--timesteps 100] [--epochs 200] [--lr 0.02] [--em-iterations 10]
                                [--particles 128] [--trajectories 128] [--seed 0]

Simulates series from the two-regime model of examples/slds_em.py, starts from slds_em_full.py's perturbed copy of ALL ten
parameters and minimises `aesmc_amd.rao_blackwell.collapsed_switching_loss` — minus the mean log-evidence of the
deterministic collapsed-mixture filter (GPB2), whose gradient the adjoint kernels K52 and K54 compute: no particles, no
smoothing pass, no sampling.  The parametrisation is the USER's, in torch ops in front of the library: softmax rows for Pi
and pi0, exp for the scales s0, q and r (shared across regimes: a leading 1), the rest free.  Any other differentiable
program — a network that produces C, a regulariser, a shared optimiser — goes in the same place.

Prints the collapsed evidence per step every few epochs, then runs EM (`switching_smooth_states`,
`switching_expected_statistics`, `switching_m_step`) from the same start on the same data and prints the same figure for
its models: one yardstick for both.  C and d are identified only up to a change of basis of the latent, which is why the
evidence is the figure to watch.
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

SCALES, ROWS = ("s0", "q", "r"), ("pi0", "Pi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--em-iterations", type=int, default=10)
    ap.add_argument("--particles", type=int, default=128)
    ap.add_argument("--trajectories", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.timesteps < 2:
        ap.error("--timesteps must be at least 2: the M-step needs a transition")

    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    D = args.dim
    truth = true_parameters(D, args.seed)
    exact = build(truth, device)
    observations = exact.simulate(args.timesteps, args.batch, seed=args.seed + 1)
    rng = np.random.default_rng(args.seed + 2)
    noisy = lambda value, scale: np.asarray(value, dtype=np.float64) + scale * rng.standard_normal(np.shape(value))
    start = dict(pi0=np.array([0.6, 0.4]), Pi=np.array([[0.7, 0.3], [0.3, 0.7]]), m0=noisy(truth["m0"], 0.3), s0=1.5,
                 A=noisy(truth["A"], 0.15), b=noisy(truth["b"], 0.3), q=np.full((1, D), 0.5), C=noisy(truth["C"], 0.1),
                 d=noisy(truth["d"], 0.1), r=np.full((1, D), 0.5))
    evidence = lambda model: rao_blackwell.collapsed_switching_filter(observations, model)["log_marginal_likelihood"] \
        .mean().item() / args.timesteps

    # ---- Adam on the collapsed evidence: the free variables and the map to the ten parameters ---------------------------------
    as_tensor = lambda value: torch.as_tensor(np.asarray(value, dtype=np.float64), device=device)
    free = {}
    for name, value in start.items():
        value = as_tensor(value).reshape(-1) if name == "s0" else as_tensor(value)
        free[name] = (torch.log(value) if name in SCALES + ROWS else value).clone().requires_grad_(True)

    def parameters():
        out = {name: value for name, value in free.items() if name not in SCALES + ROWS}
        out.update({name: torch.softmax(free[name], dim=-1) for name in ROWS})
        out.update({name: torch.exp(free[name]) for name in SCALES})
        return out

    optimiser = torch.optim.Adam(list(free.values()), lr=args.lr)
    for epoch in range(args.epochs + 1):
        loss = rao_blackwell.collapsed_switching_loss(observations, parameters())
        if epoch % max(1, args.epochs // 10) == 0 or epoch == args.epochs:
            with torch.no_grad():
                now = parameters()
            print("epoch {:4d}: collapsed log evidence per step {:9.5f}   |A - A_true| {:.4f}   q {:.3f}   r {:.3f}   Pi diagonal {}"
                  .format(epoch, -loss.item() / args.timesteps, (now["A"] - exact.A).norm().item(), now["q"].mean().item(),
                          now["r"].mean().item(), ", ".join("{:.3f}".format(v) for v in now["Pi"].diagonal().tolist())))
        if epoch == args.epochs:
            break
        optimiser.zero_grad()
        loss.backward()
        optimiser.step()
    with torch.no_grad():
        learned = rao_blackwell.SwitchingLinearGaussian(**parameters())
    by_gradient = evidence(learned)

    # ---- EM from the same start on the same data, measured by the same evidence ---------------------------------------------------
    model = build(start, device)
    for iteration in range(args.em_iterations + 1):
        print("EM iteration {:2d}: collapsed log evidence per step {:9.5f}".format(iteration, evidence(model)))
        if iteration == args.em_iterations:
            break
        out, _ = rao_blackwell.switching_smooth_states(observations, model, args.particles, num_trajectories=args.trajectories,
                                                       lookahead=True, return_trajectories=True)
        model = rao_blackwell.switching_m_step(rao_blackwell.switching_expected_statistics(out, observations, model), model)
    print("final collapsed log evidence per step: Adam {:9.5f}   EM {:9.5f}   at the true parameters {:9.5f}".format(
        by_gradient, evidence(model), evidence(exact)))


if __name__ == "__main__":
    main()
