"""Bayesian learning of the transition matrix of a switching linear-Gaussian state-space model by particle Gibbs.

    python examples/slds_gibbs.py [--dim 2] [--particles 16] [--batch 16] [--timesteps 200] [--iterations 200]
                                  [--burn-in 50] [--alpha 1.0] [--seed 0] [--lookahead] [--start smoother|collapsed]

Simulates series from a two-regime model with a known Pi, puts an independent Dirichlet(alpha, .., alpha) prior on every row of
Pi and alternates

    regimes | Pi, y   one sweep of `aesmc_amd.rao_blackwell.switching_particle_gibbs` per series (the batch rows), started from
                      the sweep before: a Rao-Blackwellised conditional particle filter with ancestor sampling (K34 backwards
                      along the reference, then K37 and K38 per step) — a kernel that leaves p(s_{0:T-1} | y, Pi) invariant for
                      any number of particles, so a handful suffices;
    Pi | regimes      row i ~ Dirichlet(alpha + the number of transitions i -> j over all series), in plain torch

— a Gibbs sampler on (regimes, Pi) whose stationary law is their joint posterior.  The other parameters are held at their true
values.  --lookahead: the sweeps are the look-ahead (fully adapted) conditional filter — the free particles resample on
p(y_t | history) and draw the regime from its exact posterior (K48 and K49 per step in place of K37 and K38).  --start
collapsed: the first reference path is the argmax of the smoothed regime probabilities of the deterministic collapsed-mixture
smoother (`collapsed_switching_smooth`: Kim's smoother, kernels K50 and K51) under the starting Pi — a good start that costs
no particles — instead of one trajectory of the particle smoother.  Prints the
posterior mean and standard deviation of Pi over the kept iterations beside the truth.
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


def transition_counts(regimes, M):
    """[M,M] float64: how often i is followed by j along the paths regimes (T tensors [batch_size, 1])."""
    paths = torch.stack(regimes).long()
    counts = torch.zeros(M, M, dtype=torch.float64, device=paths.device)
    counts.index_put_((paths[:-1].reshape(-1), paths[1:].reshape(-1)),
                      torch.ones(paths[1:].numel(), dtype=torch.float64, device=paths.device), accumulate=True)
    return counts


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--dim", type=int, default=2)
    parser.add_argument("--particles", type=int, default=16)
    parser.add_argument("--batch", type=int, default=16)
    parser.add_argument("--timesteps", type=int, default=200)
    parser.add_argument("--iterations", type=int, default=200)
    parser.add_argument("--burn-in", type=int, default=50)
    parser.add_argument("--alpha", type=float, default=1.0)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--lookahead", action="store_true")
    parser.add_argument("--start", choices=("smoother", "collapsed"), default="smoother",
                        help="the first reference path: a trajectory of the particle smoother, or the collapsed smoother's argmax")
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aesmc_amd runs on a HIP device (no CPU fallback)")
    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    truth = true_parameters(args.dim, args.seed)
    M = 2
    observations = build(truth, device).simulate(args.timesteps, args.batch, seed=args.seed)
    Pi = np.full((M, M), 1.0 / M)      # the start: no stickiness at all
    model = build(dict(truth, Pi=Pi), device)
    if args.start == "collapsed":
        # the first path: the most probable smoothed regime of Kim's smoother under the starting Pi, then the chain
        smoothed = rao_blackwell.collapsed_switching_smooth(observations, model)["smoothed_regime_probabilities"]
        path = list(smoothed.argmax(dim=-1).to(torch.int32).unbind(0))
    else:
        # the first path: one trajectory of the smoother under the starting Pi (reference=None), then the chain
        out = rao_blackwell.switching_particle_gibbs(observations, model, args.particles, 1, lookahead=args.lookahead)
        path = [regime[:, 0].contiguous() for regime in out["regimes"]]
    kept = []
    for iteration in range(args.iterations):
        out = rao_blackwell.switching_particle_gibbs(observations, model, args.particles, 1, reference=path,
                                                     lookahead=args.lookahead)
        path = [regime[:, 0].contiguous() for regime in out["regimes"]]
        counts = transition_counts(out["regimes"], M)
        Pi = torch.distributions.Dirichlet(counts + args.alpha).sample()
        model = build(dict(truth, Pi=Pi.cpu().numpy()), device)
        if iteration >= args.burn_in:
            kept.append(Pi.cpu().numpy())
        if iteration % max(args.iterations // 10, 1) == 0:
            print("iteration {:4d}  Pi = {}".format(iteration, np.array2string(Pi.cpu().numpy(), precision=3).replace("\n", "")))
    kept = np.stack(kept)
    print("posterior mean of Pi over {} iterations:\n{}".format(len(kept), np.array2string(kept.mean(axis=0), precision=3)))
    print("posterior standard deviation:\n{}".format(np.array2string(kept.std(axis=0), precision=3)))
    print("the truth:\n{}".format(np.array2string(truth["Pi"], precision=3)))


if __name__ == "__main__":
    main()
