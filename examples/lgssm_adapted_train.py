"""Learn a linear-Gaussian state-space model's transition matrix by ascending the fully adapted auxiliary particle
filter's evidence estimate (`aesmc_amd.adapted.adapted_loss`): no proposal is written and none is learned — for this model
class the filter resamples on p(y_t | x_{t-1}) and draws from p(x_t | x_{t-1}, y_t) in closed form, and its backward runs
through kernels K29 / K30.

    python examples/lgssm_adapted_train.py [--dim 4] [--particles 512] [--batch 64] [--timesteps 20] [--steps 300]

Prints the loss beside minus the Kalman filter's exact log-likelihood per sequence (what the loss estimates, from above in
expectation) and how far the learned matrix is from the one that generated the data.
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
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--particles", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    truth = models.LgssmNd(args.dim, seed=1, validate_args=False).to(device)
    model = models.LgssmNd(args.dim, seed=0, validate_args=False, affine=True).to(device)
    with torch.no_grad():                       # start from a transition that forgets too fast; C is the truth's
        model.A.mul_(0.5)
        model.C.copy_(truth.C)
    optimiser = torch.optim.Adam([model.A], lr=1e-2)
    observations = truth.simulate(args.timesteps, args.batch, seed=7)
    exact = -float(np.mean(models.kalman_log_likelihood(truth, observations)))
    for step in range(args.steps):
        optimiser.zero_grad(set_to_none=True)
        loss = aesmc.adapted.adapted_loss(observations, model.initial, model.transition, model.emission, args.particles)
        loss.backward()
        optimiser.step()
        if step % 50 == 0 or step == args.steps - 1:
            distance = float((model.A.detach() - truth.A.detach()).norm() / truth.A.detach().norm())
            print("step {:4d}: loss {:.4f} (the generating model's exact value {:.4f}), |A - A*| / |A*| = {:.3f}".format(
                step, loss.item(), exact, distance))


if __name__ == "__main__":
    main()
