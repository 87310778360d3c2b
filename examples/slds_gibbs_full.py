"""Full Bayesian learning of a switching linear-Gaussian state-space model by Gibbs sampling over regimes, states and all ten
parameters (pi0, Pi, m0, s0, A, b, q, C, d, r).

    python examples/slds_gibbs_full.py [--dim 2] [--particles 16] [--batch 16] [--timesteps 100] [--iterations 300]
                                       [--burn-in 100] [--seed 0]

Simulates series from examples/slds_gibbs.py's two-regime model, starts from a perturbed copy of every parameter and alternates
three blocks whose stationary law is the joint posterior of (s, z, theta) given y:

    s | theta, y       one sweep of `aesmc_amd.rao_blackwell.switching_particle_gibbs` per series, started from the sweep before
                       (z integrated out: K34 backwards along the reference, K37 and K38 per step);
    z | s, theta, y    `switching_sample_states`: the conditional Kalman filter forward, then the whole backward-sampling pass in
                       ONE launch (K47) — the simulation smoother;
    theta | s, z, y    conjugate, in plain torch here as slds_gibbs.py does for Pi.

The complete-data sums of the last block come from `switching_expected_statistics`: its input admits a draw in place of
moments — the states as means with ZERO covariances and ZERO cross-covariances (N = 1) — and K45 then returns exactly the sums
over t and the series of z z^T, z_t x_{t-1}^T, y x^T, .. per regime (x = (z, 1)); no plain-torch sums are formed here.

Priors, all weak and independent across regimes and rows:
    pi0 and every row of Pi    Dirichlet(1, .., 1)
    row i of [A_j b_j], q_j[i]^2      normal-inverse-gamma: q^2 ~ IG(2, 0.1), row | q^2 ~ N(0, q^2 / 0.01 I)
    row i of [C_j d_j], r_j[i]^2      normal-inverse-gamma: r^2 ~ IG(2, 0.1), row | r^2 ~ N(row i of [I 0], r^2 / 1.0 I) — centred
                                      on the identity: the latent's basis is identified by this prior alone (any invertible
                                      change of basis of z gives the same likelihood), as weakly as the data allow
    m0[i], s0[i]^2             normal-inverse-gamma: s0^2 ~ IG(2, 1), m0 | s0^2 ~ N(0, s0^2 / 0.01)
With sufficient statistics n, G = sum x x^T, g = sum target x, h = sum target^2 of a row's regression on x the posterior is
NIG with Lam = Lam0 + G, w = Lam^-1 (Lam0 w0 + g), a = a0 + n / 2, b = b0 + (h + w0^T Lam0 w0 - w^T Lam w) / 2.

Prints the posterior mean and standard deviation of every parameter over the kept iterations beside the truth, how many of
the scalar parameters lie within three standard deviations of their posterior mean, and the same for C_j A_j C_j^-1, which
no change of basis of the latent moves (the entries of A, b, q, C and d themselves are held in place by the prior on C only:
over a few hundred iterations the chain stays near the basis it started in; over a thousand the scale of z drifts — C grows,
q shrinks, A's off-diagonal entries move — while Pi, r and C A C^-1 stay where the data put them).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import aesmc_amd as aesmc  # noqa: F401
from aesmc_amd import rao_blackwell
from slds_gibbs import build, true_parameters

KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")


def nig_rows(gram, cross, square, count, mean0, precision0, shape0, rate0, generator):
    """A draw of (rows [R, X], variances [R]) of R independent regressions that share the regressors' gram [X, X]: cross
    [R, X] = sum target x^T, square [R] = sum target^2, count = n; the prior's mean0 [R, X], precision0 (times I), shape0 and
    rate0.  float64 on the CPU."""
    X = gram.size(0)
    lam = gram + precision0 * torch.eye(X, dtype=torch.float64)
    factor = torch.linalg.cholesky(lam)
    mean = torch.cholesky_solve((precision0 * mean0 + cross).t(), factor).t()                      # [R, X]
    rate = rate0 + 0.5 * (square + precision0 * (mean0 * mean0).sum(dim=1) - ((mean @ lam) * mean).sum(dim=1))
    shape = shape0 + 0.5 * count
    variance = rate.clamp_min(1e-300) / torch.distributions.Gamma(shape, 1.0).sample((mean.size(0),)).to(torch.float64)
    eps = torch.randn(mean.shape, dtype=torch.float64, generator=generator)
    # row = mean + sigma L^-T eps: covariance sigma^2 Lam^-1
    rows = mean + variance.sqrt().unsqueeze(1) * torch.linalg.solve_triangular(factor.t(), eps.t(), upper=True).t()
    return rows, variance


def draw_parameters(statistics, M, D, Dy, generator):
    """theta | s, z, y from the complete-data sums (`switching_expected_statistics` of a draw): a dict of numpy arrays."""
    s = {key: value.cpu() for key, value in statistics.items() if torch.is_tensor(value)}
    dirichlet = lambda counts: torch.distributions.Dirichlet(counts + 1.0).sample()
    out = {"pi0": dirichlet(s["initial_counts"]), "Pi": torch.stack([dirichlet(row) for row in s["transition_counts"]])}
    first = s["initial_state"]                                                                       # sum x_0 x_0^T, [X, X]
    rows, variance = nig_rows(first[D:, D:], first[:D, D:], torch.diagonal(first)[:D], first[D, D],
                              torch.zeros(D, 1, dtype=torch.float64), 0.01, 2.0, 1.0, generator)
    out["m0"], out["s0"] = rows[:, 0], variance.sqrt()
    identity = torch.cat([torch.eye(Dy, D, dtype=torch.float64), torch.zeros(Dy, 1, dtype=torch.float64)], dim=1)
    A, b, q, C, d, r = [], [], [], [], [], []
    for j in range(M):
        rows, variance = nig_rows(s["prev_prev"][j], s["next_prev"][j], torch.diagonal(s["next_next"][j]), s["prev_prev"][j][D, D],
                                  torch.zeros(D, D + 1, dtype=torch.float64), 0.01, 2.0, 0.1, generator)
        A.append(rows[:, :D]), b.append(rows[:, D]), q.append(variance.sqrt())
        gram = s["state_state"][j, 0]                   # (no mask: one gram for every component)
        rows, variance = nig_rows(gram, s["obs_state"][j], s["obs_obs"][j], gram[D, D], identity, 1.0, 2.0, 0.1, generator)
        C.append(rows[:, :D]), d.append(rows[:, D]), r.append(variance.sqrt())
    out.update(A=torch.stack(A), b=torch.stack(b), q=torch.stack(q), C=torch.stack(C), d=torch.stack(d), r=torch.stack(r))
    return {key: value.numpy() for key, value in out.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--dim", type=int, default=2)
    parser.add_argument("--particles", type=int, default=16)
    parser.add_argument("--batch", type=int, default=16)
    parser.add_argument("--timesteps", type=int, default=100)
    parser.add_argument("--iterations", type=int, default=300)
    parser.add_argument("--burn-in", type=int, default=100)
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aesmc_amd runs on a HIP device (no CPU fallback)")
    if args.timesteps < 2:
        parser.error("--timesteps must be at least 2: the draw of A, b, q needs a transition")
    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    generator = torch.Generator().manual_seed(args.seed)
    D, M = args.dim, 2
    truth = true_parameters(D, args.seed)
    observations = build(truth, device).simulate(args.timesteps, args.batch, seed=args.seed)
    full = lambda value, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), shape))
    truth = dict(truth, s0=full(truth["s0"], (D,)), q=full(truth["q"], (M, D)), C=full(truth["C"], (M, D, D)),
                 d=full(truth["d"], (M, D)), r=full(truth["r"], (M, D)))
    rng = np.random.default_rng(args.seed + 2)
    noisy = lambda value, scale: np.asarray(value, dtype=np.float64) + scale * rng.standard_normal(np.shape(value))
    parameters = dict(pi0=np.array([0.6, 0.4]), Pi=np.array([[0.7, 0.3], [0.3, 0.7]]), m0=noisy(truth["m0"], 0.3),
                      s0=np.full(D, 1.5), A=noisy(truth["A"], 0.1), b=noisy(truth["b"], 0.2), q=np.full((M, D), 0.5),
                      C=noisy(truth["C"], 0.05), d=noisy(truth["d"], 0.1), r=np.full((M, D), 0.5))
    model = build(parameters, device)
    out = rao_blackwell.switching_particle_gibbs(observations, model, args.particles, 1)
    path = [regime[:, 0].contiguous() for regime in out["regimes"]]
    zeros = [torch.zeros(args.batch, 1, D * (D + 1) // 2, dtype=torch.float64, device=device)] * args.timesteps
    no_cross = [torch.zeros(args.batch, 1, D, D, dtype=torch.float64, device=device)] * (args.timesteps - 1)
    kept = []
    for iteration in range(args.iterations):
        out = rao_blackwell.switching_particle_gibbs(observations, model, args.particles, 1, reference=path)
        path = [regime[:, 0].contiguous() for regime in out["regimes"]]
        regimes = [regime.to(torch.int32) for regime in out["regimes"]]
        states = rao_blackwell.switching_sample_states(observations, model, regimes)["states"]
        statistics = rao_blackwell.switching_expected_statistics(
            {"regimes": regimes, "means": states, "covariances": zeros, "cross_covariances": no_cross}, observations, M)
        parameters = draw_parameters(statistics, M, D, D, generator)
        model = build(parameters, device)
        if iteration >= args.burn_in:
            kept.append(parameters)
        if iteration % max(args.iterations // 10, 1) == 0:
            print("iteration {:4d}  Pi = {}  |A - truth| = {:.3f}  q = {}".format(
                iteration, np.array2string(parameters["Pi"], precision=3).replace("\n", ""),
                float(np.abs(parameters["A"] - truth["A"]).max()), np.array2string(parameters["q"], precision=3).replace("\n", "")))
    inside = total = 0
    for key in KEYS:
        draws = np.stack([sample[key] for sample in kept])
        mean, deviation = draws.mean(axis=0), draws.std(axis=0)
        covered = np.abs(mean - truth[key]) <= 3.0 * deviation
        inside, total = inside + int(covered.sum()), total + covered.size
        flat = lambda value: np.array2string(np.asarray(value).reshape(-1), precision=3, max_line_width=200)
        print("{:>3}  posterior mean {}\n     posterior sd   {}\n     the truth      {}".format(key, flat(mean), flat(deviation),
                                                                                                flat(truth[key])))
    print("{} of {} scalar parameters lie within 3 posterior standard deviations of the posterior mean ({} kept iterations)"
          .format(inside, total, len(kept)))
    # A, b, q, C and d move together under a change of basis of the latent, which only the prior on C holds in place;
    # C_j A_j C_j^-1 — the transition as the observations see it — does not depend on the basis
    seen = lambda sample: np.stack([sample["C"][j] @ sample["A"][j] @ np.linalg.inv(sample["C"][j]) for j in range(M)])
    draws = np.stack([seen(sample) for sample in kept])
    mean, deviation = draws.mean(axis=0), draws.std(axis=0)
    covered = np.abs(mean - seen(truth)) <= 3.0 * deviation
    flat = lambda value: np.array2string(np.asarray(value).reshape(-1), precision=3, max_line_width=200)
    print("C A C^-1  posterior mean {}\n          posterior sd   {}\n          the truth      {}\n          {} of {} within 3 sd"
          .format(flat(mean), flat(deviation), flat(seen(truth)), int(covered.sum()), covered.size))


if __name__ == "__main__":
    main()
