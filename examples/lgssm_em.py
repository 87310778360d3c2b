"""EM for the transition matrix of a d-dimensional linear-Gaussian state-space model from the two-slice particle smoother:

    A = (sum_t E[x_{t+1} x_t^T | y]) (sum_t E[x_t x_t^T | y])^-1

the lag-one cross moments from `aesmc_amd.smoothing.two_slice_smooth` (kernel K23; `previous = following = None`: the latent
itself), the second moments from `statistics.empirical_expectation` under the smoothed weights the same pass returns.

    python examples/lgssm_em.py [--dim 3] [--particles 256] [--batch 64] [--timesteps 20] [--steps 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import aesmc_amd as aesmc
from aesmc_amd.testing import models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    truth = models.LgssmNd(args.dim, seed=1, validate_args=False).to(device)
    observations = truth.simulate(args.timesteps, args.batch, seed=7)
    model = models.LgssmNd(args.dim, seed=1, validate_args=False).to(device)
    with torch.no_grad():
        model.A.copy_(0.5 * torch.eye(args.dim, device=device))          # a poor start; everything else is the truth's
    outer = lambda x: x.unsqueeze(-1) * x.unsqueeze(-2)                  # [B,d] -> [B,d,d]
    for step in range(args.steps + 1):
        print("step {}: |A - truth| = {:.4f}".format(step, (model.A - truth.A).abs().max().item()))
        if step == args.steps:
            break
        model.tune_proposal()                                            # the locally optimal proposal of the current A
        with torch.no_grad():
            latents, smoothed, cross, log_z = aesmc.smoothing.two_slice_smooth(
                observations, model.initial, model.transition, model.emission, model.proposal, args.particles)
            lagged = sum(c.double().sum(dim=0) for c in cross)           # sum_t sum_b E[x_{t+1} x_t^T]: [d,d]
            second = sum(aesmc.statistics.empirical_expectation(torch.as_tensor(x), w, outer).double().sum(dim=0)
                         for x, w in zip(latents[:-1], smoothed[:-1]))   # sum_t sum_b E[x_t x_t^T]
            model.A.copy_((lagged @ torch.linalg.inv(second)).to(model.A.dtype))
        print("        log Z per sequence {:.3f}".format(log_z.mean().item()))
    print("estimate\n{}\ntruth\n{}".format(model.A.detach().cpu().numpy().round(3), truth.A.detach().cpu().numpy().round(3)))


if __name__ == "__main__":
    main()
