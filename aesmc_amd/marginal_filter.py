"""The marginal particle filter (Klaas, de Freitas & Doucet 2005), the estimator behind `infer("mpf", ...)` and the
training objective `losses.get_loss(..., algorithm="vmpf")` (Lai, Domke & Sheldon 2022, "Variational marginal particle
filters").

It keeps the SMC draw — resample an ancestor, then propose from it — and weights the new particle against the whole
predictive mixture instead of against its one sampled ancestor:

    v_t[k] = g(y_t | x_t[k]) * sum_i w_{t-1}[i] f(x_t[k] | x_{t-1}[i]) / sum_i w_{t-1}[i] q(x_t[k] | x_{t-1}[i], y_t)
    Z      = prod_t (1/K) sum_k v_t[k]

Z is unbiased; every weight is the Rao-Blackwellisation of the SMC weight over the ancestor choice, so its variance is never
larger; and the log-weights depend on ALL of step t-1's particles and weights through two smooth log-sum-exps, so the
gradient reaches earlier weights and particles without a score-function term for the resampling step.

With a Normal transition and proposal whose scales do not vary over batch or particle — what `smoothing` covers — both
mixture sums are one launch of kernel K22 each (`_ops.pairwise_lse`), their backward two launches of K25 each.

THE COST IS QUADRATIC in the number of particles: O(batch_size num_particles^2 D) per step, in float64, forwards and again
(about three times) backwards.  It is meant for num_particles in the hundreds: at batch_size = 1024, num_particles = 512,
T = 100 the forward alone is 2 * 99 * 1024 * 512^2 = 5e10 pairs; at num_particles = 4096 a single K22 launch of 64 batch
rows takes 40 ms (profiles/ffbsm_pairwise_lse.txt, profiles/mpf_pairwise_pass.txt).

The reference has no counterpart; this module adds to its interface and changes none of it.
"""
import numpy as np
import torch

from . import _kernels
from . import _ops
from . import inference
from . import smoothing
from . import state

_COVERED = ("covered: a transition and a proposal (from time 1 on) that return an AffineNormal or a "
            "torch.distributions.Normal in FULLY_EXPANDED batch-shape mode, the location shaped like the latent "
            "[batch_size, num_particles, ...] with at most {} values per particle, the scale one value or one per latent "
            "dimension (not varying over batch or particle, by shape or zero strides); tensor latents of float32 or "
            "float64; Markov models".format(smoothing.MAX_LATENT_DIM))


def _refuse(what):
    raise NotImplementedError("aesmc_amd.marginal_filter: {} is not implemented by the marginal particle filter; {}"
                              .format(what, _COVERED))


def _log_scales(scale, dim):
    """sum_d log scale[d] over the latent's `dim` values, a 0-dim tensor (differentiable in the scale)."""
    return torch.log(scale).sum() * (dim // scale.numel())


def run(observations, initial, transition, emission, proposal, num_particles, return_log_marginal_likelihood=False,
        return_latents=True, return_original_latents=False, return_log_weight=True, return_log_weights=False,
        return_ancestral_indices=False, resampling=None):
    """The body of `inference.infer("mpf", ...)`: the callables' contract, the return dict, the `return_*` flags,
    `resampling=`, the uniform feeds and the deferred flags are `infer`'s.

    Step 0 is `infer`'s ordinary first step.  Every step t >= 1, MARKOV MODELS ONLY (`previous_latents[-1]` must be all
    of the latents a callable reads): each callable is called ONCE, on the stored, un-resampled particles —
        proposal(previous_latents=originals[:t], time=t, observations=observations)                      -> loc_q, s_q
        transition(previous_latents=originals[:t], time=t, previous_observations=observations[:t])       -> loc_f, s_f
        emission(latents=originals[:t+1], time=t, previous_observations=observations[:t])                 (any emission)
    the ancestor indices come from the resampling launch on log_weights[t-1] with the scheme in force, the draw is
    x_t = loc_q[ancestor] + s_q * eps (reparameterised, eps from the source `state.sample` uses; the gradient goes through
    the gather, not through the indices), and
        log v_t = log g(y_t | x_t) + ( (pairwise_lse(x_t, loc_f, s_f, log_v_{t-1}) - sum_d log s_f[d])
                                     - (pairwise_lse(x_t, loc_q, s_q, log_v_{t-1}) - sum_d log s_q[d]) )
    ((2 pi)^(D/2) and any constant in log_v_{t-1} cancel).  A proposal that returns the transition's own location and scale
    makes the bracket exactly zero: log v_t == log g, bit for bit.  log Z = sum_t (logsumexp_k log v_t - log K).

    `latents` (with return_latents) is the genealogy along the ancestors the draws were proposed from, as under 'smc'.
    Quadratic in num_particles (see the module's docstring).  Anything not covered raises NotImplementedError before the
    step's launches; not capturable into a hipGraph."""
    stratified = inference._resolve_resampling(resampling) == "stratified"
    num_timesteps = len(observations)
    if any(isinstance(observation, dict) for observation in observations):
        _refuse("dict observations")
    batch_size = observations[0].size(0)
    provider = _kernels.get()
    originals, indices, log_weights, step_lse = [], [], [], []
    feed = None

    for time in range(num_timesteps):
        if time == 0:
            proposal_dist = proposal(time=0, observations=observations)
            if isinstance(proposal_dist, dict):
                _refuse("dict latents")
            latent = state.materialise_draw(state.sample(proposal_dist, batch_size, num_particles))
            if isinstance(latent, dict) or not torch.is_tensor(latent):
                _refuse("dict latents")
            if latent.dtype not in (torch.float32, torch.float64):
                _refuse("latents of dtype {}".format(latent.dtype))
            originals.append(latent)
            emission_dist = emission(latents=originals, time=0)
            log_q = state.log_prob(proposal_dist, latent)
            log_p = state.log_prob(initial(), latent)
            log_g = state.log_prob(emission_dist, state.expand_observation(observations[0], num_particles))
            log_weight, lse = _ops.logweight_lse(log_p, log_g, log_q)
        else:
            previous, stored = log_weights[-1], originals[-1]
            history = list(originals)
            proposal_dist = proposal(previous_latents=history, time=time, observations=observations)
            loc_q, scale_q = smoothing._normal_terms(proposal_dist, stored, _refuse, what="proposal", detach=False)
            transition_dist = transition(previous_latents=history, time=time, previous_observations=observations[:time])
            loc_f, scale_f = smoothing._normal_terms(transition_dist, stored, _refuse, what="transition", detach=False)
            if not (provider.pairwise_lse_covers(loc_q, loc_q, scale_q, previous) and
                    provider.pairwise_lse_covers(loc_f, loc_f, scale_f, previous)):
                _refuse("these log-weights, locations and scales together (one dtype, float32 or float64, on one device)")
            if feed is None:
                feed = inference._FEED_OVERRIDE.get() or (
                    inference._StratifiedFeed(batch_size, num_particles, previous.device) if stratified else
                    inference._UniformFeed(batch_size, num_timesteps - 1, previous.device))
            uniforms = feed.next()
            per_particle = uniforms.dim() == 2 and tuple(uniforms.shape) == tuple(previous.shape)
            if per_particle != stratified and num_particles != 1:
                raise ValueError("aesmc_amd: {} resampling takes {} uniforms per step, the feed returned {}".format(
                    "stratified" if stratified else "systematic",
                    "[batch_size, num_particles]" if stratified else "[batch_size]", tuple(uniforms.shape)))
            index, _, _ = _ops.resample_step(previous.detach(), uniforms)
            indices.append(index)
            dim = 1
            for size in stored.shape[2:]:
                dim *= size
            noise = state._standard_normal(stored.shape, stored.dtype, stored.device)
            spread = scale_q if scale_q.numel() == 1 else scale_q.reshape(stored.shape[2:])
            latent = _ops.resample_gather(loc_q, index) + spread * noise
            originals.append(latent)
            emission_dist = emission(latents=originals, time=time, previous_observations=observations[:time])
            log_g = state.log_prob(emission_dist, state.expand_observation(observations[time], num_particles))
            mixture_f = _ops.pairwise_lse(latent, loc_f, scale_f, previous) - _log_scales(scale_f, dim)
            mixture_q = _ops.pairwise_lse(latent, loc_q, scale_q, previous) - _log_scales(scale_q, dim)
            # (this order: identical operands give mixture_f - mixture_q == 0 exactly, and log v == log g bit for bit)
            log_weight, lse = _ops.logweight_lse(log_g, mixture_f - mixture_q)
        log_weights.append(log_weight)
        step_lse.append(lse)

    device = log_weights[-1].device
    log_marginal_likelihood = latents = None
    if return_log_marginal_likelihood:
        log_marginal_likelihood = torch.sum(torch.stack(step_lse, dim=0) - np.log(num_particles), dim=0)
    if return_latents:
        latents = inference.get_resampled_latents(originals, indices)
    capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
    if not capturing:
        inference._raise_for_flags(provider.read_flags(device))
    return {"log_marginal_likelihood": log_marginal_likelihood,
            "latents": latents,
            "original_latents": originals if return_original_latents else None,
            "log_weight": log_weights[-1] if return_log_weight else None,
            "log_weights": log_weights if return_log_weights else None,
            "ancestral_indices": indices if return_ancestral_indices else None,
            "last_latent": originals[-1]}
