"""Filter a switching linear-Gaussian state-space model with the Rao-Blackwellised particle filter
(`aesmc_amd.rao_blackwell.switching_filter`): only the regime is sampled, every particle carries the exact Kalman mean and
covariance of the continuous state given its regime history (kernel K31).

    python examples/slds_filter.py [--regimes 2] [--dim 2] [--particles 256] [--batch 8] [--timesteps 200] [--short 6]
                                   [--lookahead | --discrete] [--smooth] [--missing FRACTION] [--forecast H] [--collapsed]

Simulates a series whose regimes differ in their dynamics, filters it, and prints how often the most probable filtered
regime is the true one and the error of the filtered mean; then, for a short series, log Z-hat beside the exact log p(y)
from the enumeration of all M^T regime sequences.  With --lookahead the filter is `adapted_switching_filter`: every step
resamples on the exact p(y_t | history) and draws the regime from its exact posterior (kernels K32 and K33).  With
--discrete it is `discrete_switching_filter` (Fearnhead & Clifford 2003; kernels K43 and K44): no regime is drawn, every
particle proposes all M successors and K of the K M candidates survive under optimal resampling — no regime history twice,
and log Z-hat of the short series is exact once M^T <= K.  With
--smooth the stored systems are smoothed by Rao-Blackwellised backward simulation (`switching_backward_simulate`, kernels
K34 and K35) and the accuracy of the most probable SMOOTHED regime, which has seen the whole series, is printed beside the
filtered one; then the continuous state is smoothed along the drawn trajectories (`switching_state_smooth`, kernel K36) and
the error of the smoothed state mean is printed beside the filtered one's.  With --missing FRACTION every component of
every observation is dropped with that probability (NaN is written over it) and the filter runs once more with
`observed=` (the masked kernels K39 / K40): regime accuracy and state RMSE beside the fully observed run's.  With
--forecast H the last H steps are held out, the filter runs on the rest and `switching_forecast` predicts them: the RMSE
of the forecast's observation mean against the held-out observations, beside their own spread and the forecast's.
With --collapsed the deterministic collapsed-mixture filters (`collapsed_switching_filter`: GPB2 / Kim's filter and IMM, kernel
K50) and Kim's smoother (`collapsed_switching_smooth`, kernel K51) run on the same series — no particles, no random numbers
— and their evidence, regime accuracy and state RMSE are printed beside the particle filter's; for the short series their
evidence stands beside the exact one.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import aesmc_amd as aesmc  # noqa: F401
from aesmc_amd import rao_blackwell
from aesmc_amd.testing import rao_blackwell as contract


def make_model(M, D, seed):
    """Sticky regimes that rotate the state at different speeds and shrink it differently; the state is seen whole."""
    rng = np.random.default_rng(seed)
    Pi = np.full((M, M), 0.05 / max(M - 1, 1)) + (0.95 - 0.05 / max(M - 1, 1)) * np.eye(M) if M > 1 else np.ones((1, 1))
    A = np.stack([np.linalg.qr(rng.standard_normal((D, D)))[0] * (0.5 + 0.45 * i / max(M - 1, 1)) for i in range(M)])
    b = np.stack([np.full(D, 0.5 * i) for i in range(M)])
    return rao_blackwell.SwitchingLinearGaussian(np.full(M, 1.0 / M), Pi / Pi.sum(axis=1, keepdims=True), np.zeros(D), 1.0, A,
                                                 b, np.full((1, D), 0.3), np.eye(D)[None], np.zeros((1, D)),
                                                 np.full((1, D), 0.3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regimes", type=int, default=2)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--timesteps", type=int, default=200)
    ap.add_argument("--short", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lookahead", action="store_true", help="the fully adapted filter: regimes from their exact posterior")
    ap.add_argument("--discrete", action="store_true",
                    help="the discrete particle filter: all successors proposed, optimal resampling, no history twice")
    ap.add_argument("--smooth", action="store_true", help="also smooth: regime accuracy given the whole series")
    ap.add_argument("--trajectories", type=int, default=None, help="backward trajectories per series (default: --particles)")
    ap.add_argument("--missing", type=float, default=0.0, metavar="FRACTION",
                    help="also filter with every component dropped with this probability")
    ap.add_argument("--forecast", type=int, default=0, metavar="H", help="also hold out the last H steps and forecast them")
    ap.add_argument("--collapsed", action="store_true",
                    help="also run the deterministic collapsed-mixture filters (GPB2 / Kim, IMM) and Kim's smoother: the baseline")
    args = ap.parse_args()
    if args.lookahead and args.discrete:
        ap.error("--lookahead and --discrete name two filters: give one")

    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    model = make_model(args.regimes, args.dim, args.seed).to(device)
    observations, regimes, states = model.simulate(args.timesteps, args.batch, seed=args.seed + 1, return_latents=True)
    run = rao_blackwell.adapted_switching_filter if args.lookahead else \
        rao_blackwell.discrete_switching_filter if args.discrete else rao_blackwell.switching_filter
    out = run(observations, model, args.particles, return_moments=True)
    guess = out["regime_probabilities"].argmax(dim=-1)
    accuracy = (guess == torch.stack(regimes)).double().mean().item()
    error = (out["filtered_mean"] - torch.stack(states)).pow(2).mean().sqrt().item()
    print("T = {}, {} series, K = {}: filtered regime = true regime {:.1%} of the time; RMSE of the filtered mean {:.3f}; "
          "log Z-hat per step {:.4f}".format(args.timesteps, args.batch, args.particles, accuracy, error,
                                             out["log_marginal_likelihood"].mean().item() / args.timesteps))
    if args.collapsed:
        truth, latent = torch.stack(regimes), torch.stack(states)
        for label, baseline in (("GPB2 / Kim (order 2)", rao_blackwell.collapsed_switching_filter(observations, model, order=2)),
                                ("IMM (order 1)", rao_blackwell.collapsed_switching_filter(observations, model, order=1))):
            print("collapsed {}: filtered regime = true regime {:.1%} of the time; RMSE of the filtered mean {:.3f}; approximate "
                  "log p(y) per step {:.4f}".format(
                      label, (baseline["regime_probabilities"].argmax(dim=-1) == truth).double().mean().item(),
                      (baseline["filtered_mean"] - latent).pow(2).mean().sqrt().item(),
                      baseline["log_marginal_likelihood"].mean().item() / args.timesteps))
        kim = rao_blackwell.collapsed_switching_smooth(observations, model)
        print("collapsed smoother (Kim): smoothed regime = true regime {:.1%} of the time; RMSE of the smoothed mean {:.3f}".format(
            (kim["smoothed_regime_probabilities"].argmax(dim=-1) == truth).double().mean().item(),
            (kim["smoothed_mean"] - latent).pow(2).mean().sqrt().item()))
    if args.smooth:
        smoothed = rao_blackwell.switching_backward_simulate(out, model, observations, num_trajectories=args.trajectories)
        guess = smoothed["smoothed_regime_probabilities"].argmax(dim=-1)
        print("smoothed regime = true regime {:.1%} of the time (filtered: {:.1%}); {} backward trajectories per series".format(
            (guess == torch.stack(regimes)).double().mean().item(), accuracy, smoothed["regimes"][0].size(1)))
        state = rao_blackwell.switching_state_smooth(observations, model, smoothed["regimes"])
        print("RMSE of the smoothed state mean {:.3f} (filtered: {:.3f})".format(
            (state["smoothed_mean"] - torch.stack(states)).pow(2).mean().sqrt().item(), error))
    if args.missing > 0:
        observed = [torch.rand(y.shape, device=device) >= args.missing for y in observations]
        holes = [torch.where(seen, y, torch.full_like(y, float("nan"))) for y, seen in zip(observations, observed)]
        gappy = run(holes, model, args.particles, return_moments=True, observed=observed)
        guess = gappy["regime_probabilities"].argmax(dim=-1)
        print("with {:.0%} of the components missing: filtered regime = true regime {:.1%} of the time (fully observed: {:.1%}); "
              "RMSE of the filtered mean {:.3f} (fully observed: {:.3f})".format(
                  1.0 - torch.stack(observed).double().mean().item(), (guess == torch.stack(regimes)).double().mean().item(),
                  accuracy, (gappy["filtered_mean"] - torch.stack(states)).pow(2).mean().sqrt().item(), error))
    if 0 < args.forecast < args.timesteps:
        H = args.forecast
        ahead = rao_blackwell.switching_forecast(run(observations[:-H], model, args.particles), model, H)
        held = torch.stack(observations[-H:])
        spread = torch.diagonal(ahead["observation_covariance"], dim1=-2, dim2=-1).mean().sqrt().item()
        print("forecast of the last {} steps: RMSE of the observation mean {:.3f} (the held-out observations' own spread {:.3f}, "
              "the forecast's standard deviation {:.3f})".format(
                  H, (ahead["observation_mean"] - held).pow(2).mean().sqrt().item(), held.std().item(), spread))
    short = [y[:1] for y in observations[:args.short]]
    ops = {name: value.cpu().numpy() for name, value in model.operands().items()}
    exact = contract.exact_log_likelihood(ops, [y.cpu().numpy() for y in short])[0]
    repeats = [run(short, model, args.particles)["log_marginal_likelihood"].item()
               for _ in range(5)]
    print("T = {}: exact log p(y) = {:.6f} ({} regime sequences); log Z-hat over 5 runs: {}".format(
        args.short, exact, args.regimes ** args.short, ", ".join("{:.6f}".format(v) for v in repeats)))
    if args.collapsed:
        print("T = {}: collapsed log p(y): order 2 {:.6f}, order 1 {:.6f} (deterministic, approximate)".format(
            args.short, *[rao_blackwell.collapsed_switching_filter(short, model, order=order)["log_marginal_likelihood"].item()
                          for order in (2, 1)]))


if __name__ == "__main__":
    main()
