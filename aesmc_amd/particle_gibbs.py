"""Particle Gibbs: a Markov kernel on whole trajectories that leaves p(x_0..x_{T-1} | y_0..y_{T-1}) invariant for ANY
number of particles (Andrieu, Doucet & Holenstein 2010), with ancestor sampling (PGAS; Lindsten, Jordan & Schoen 2014).

`conditional_smc` is one sweep: an SMC run whose last particle slot, K-1, is pinned to a reference path x'_0..x'_{T-1},
followed by one draw of a path from the final weights along the ancestors.  Handing the result back in as the next
reference gives a Markov chain on paths whose stationary law is the joint smoothing distribution exactly — the particles
only decide how fast it mixes.  `particle_gibbs` runs that chain, batch rows being independent chains.

Ancestor sampling re-draws, at every step, which particle the pinned slot descends from, in proportion to

    exp(log_weights[t][b,j]) * transition(x'_{t+1} | latents[t][b,j])

(the backward-simulation weight of `smoothing.backward_simulate`, for one trajectory), so the reference path is broken
into pieces and the early states are replaced at every sweep: K = 8 .. 64 particles mix where plain conditional SMC,
whose paths all coalesce onto the reference going back in time, needs thousands.  A sweep costs O(K) per step.

Resampling is MULTINOMIAL, unlike `infer`'s systematic or stratified: for those, pinning a slot is not a valid
conditional resampling without extra machinery (Chopin & Singh 2015); for multinomial the simple conditional step is
exact.  One launch of kernel K26 per step (`aesmc_conditional_ancestor_index`) draws the K-1 free ancestors and the
pinned slot's in one go.

This is what to reach for when moving from filtering to learning: the sampling step of particle Gibbs over parameters,
of particle stochastic-approximation EM, of Monte-Carlo EM — all built on top of `particle_gibbs`, none of them here.

The reference has no counterpart; this module adds to its interface and changes none of it.
"""
import torch

from . import _kernels
from . import _lazy
from . import _ops
from . import _syncfree
from . import inference
from . import smoothing
from . import state

_COVERED = ("covered: tensor latents of float32 or float64 with at most {} particles; with ancestor_sampling=True, "
            "Markov models whose transition returns an AffineNormal or a torch.distributions.Normal in FULLY_EXPANDED "
            "batch-shape mode, its location shaped like the latent [batch_size, num_particles, ...] with at most {} values "
            "per particle, its scale one value or one per latent dimension (not varying over batch or particle, by shape "
            "or zero strides)".format(_kernels.HipKernels.CONDITIONAL_MAX_PARTICLES, smoothing.MAX_LATENT_DIM))


def _refuse(what):
    raise NotImplementedError("aesmc_amd.particle_gibbs: {} is not implemented; {}".format(what, _COVERED))


def conditional_smc(observations, initial, transition, emission, proposal, num_particles, reference,
                    ancestor_sampling=True, uniforms=None, return_particles=False):
    """One sweep of conditional SMC: a new path given `reference`, from a kernel that leaves the joint smoothing
    distribution invariant.

    observations, initial, transition, emission, proposal, num_particles: as `inference.infer("smc", ...)` takes them, and
        the callables are called exactly as it calls them — `previous_latents` is the RESAMPLED history of the particles
        (a sequence whose entries are gathered when read), so a model written for `infer` runs unchanged.
    reference: T tensors [batch_size, ...], one path per batch row, in the latents' shape (without the particle dim) and
        dtype.  Slot num_particles - 1 of every step's particles is overwritten with it before any density is taken.
    ancestor_sampling: True — at every step t >= 1 the transition is called ONCE more, on the stored, un-resampled
        particles, as `transition(previous_latents=latents[:t], time=t, previous_observations=observations[:t])` with
        plain tensors, and the pinned slot's ancestor is drawn in proportion to weight x transition density to
        reference[t].  MARKOV MODELS ONLY: `previous_latents[-1]` must be all of the latents the transition reads.
        Covered and refused as in `smoothing.backward_simulate`.  False — the pinned slot keeps ancestor
        num_particles - 1 (plain conditional SMC); any transition `state.log_prob` takes is allowed.
    uniforms: None — one `torch.rand((batch_size, num_particles), dtype=torch.float64)` block per resampling step on the
        particles' device and a [batch_size, 1] block for the final draw, from torch's generator for that device (seed
        with torch.manual_seed); numpy's RandomState is not consumed.  Or a length-T sequence of float64 device tensors:
        `uniforms[t]` [batch_size, num_particles] for t <= T-2 — the ancestors of step t+1, drawn from step t's weights
        (column k is slot k's) — and `uniforms[T-1]` [batch_size, 1] for the final draw (replay).  Inside
        `distributed.shard_scope`, None raises NotImplementedError (as `backward_simulate` does: the device draws have no
        global block that every rank could cut its rows from).
    return_particles: also return a dict with `latents` (T x [batch_size, num_particles, ...], the particles as drawn
        with the reference in slot num_particles - 1), `log_weights` (T x [batch_size, num_particles]),
        `ancestral_indices` ((T-1) x int64 [batch_size, num_particles]) and `indices` (T x int64 [batch_size]: the slot
        the new path passes through).

    Returns T tensors [batch_size, ...], the new path, detached.  With `return_particles`: (path, particles).

    Every slot, the pinned one included, is weighted transition x emission / proposal under its own ancestor.  Per step:
    the extra transition call (ancestor sampling), one launch of K26, the gathers the callables ask for, the draw, the
    densities and K1.  At the end one categorical draw per row from the last weights (K21 without a transition term) and a
    walk back through the ancestors.

    num_particles above 8192, dict latents, a reference of another length, shape or dtype raise NotImplementedError or
    ValueError before the first resampling launch.  NaN log-weights or locations raise FloatingPointError, a row without
    a finite maximum RuntimeError — read once, at the end (one synchronisation per call); an exception on the way
    discards whatever was flagged.  Runs under torch.no_grad(); not capturable into a hipGraph."""
    num_timesteps = len(observations)
    num_particles = int(num_particles)
    if num_timesteps == 0 or len(reference) != num_timesteps:
        raise ValueError("conditional_smc: reference must hold one tensor per timestep ({}), got {}".format(
            num_timesteps, len(reference)))
    if num_particles < 1:
        raise ValueError("conditional_smc: num_particles must be at least 1")
    if num_particles > _kernels.HipKernels.CONDITIONAL_MAX_PARTICLES:
        _refuse("num_particles = {}".format(num_particles))
    if any(isinstance(x, dict) for x in reference) or any(isinstance(x, dict) for x in observations):
        _refuse("dict latents or observations")
    batch_size = observations[0].size(0)
    for time, x in enumerate(reference):
        if not torch.is_tensor(x) or x.dim() < 1 or x.size(0) != batch_size:
            raise ValueError("conditional_smc: reference[{}] must be a tensor [{}, ...]".format(time, batch_size))
    if uniforms is None:
        from . import distributed
        if distributed.active_shard() is not None:
            raise NotImplementedError(
                "aesmc_amd: conditional_smc inside distributed.shard_scope draws its uniforms on the device, where no "
                "global block exists that every rank could cut its rows from. Pass uniforms= (one [batch_size, "
                "num_particles] float64 block per resampling step and a [batch_size, 1] block for the final draw).")
    elif len(uniforms) != num_timesteps:
        raise ValueError("conditional_smc: uniforms must hold one block per timestep ({}), got {}".format(
            num_timesteps, len(uniforms)))
    provider = _kernels.get()
    pinned = num_particles - 1

    def block(time, device):
        columns = 1 if time == num_timesteps - 1 else num_particles
        if uniforms is None:
            return torch.rand((batch_size, columns), dtype=torch.float64, device=device)
        u = uniforms[time]
        if not torch.is_tensor(u) or tuple(u.shape) != (batch_size, columns) or u.dtype != torch.float64:
            raise ValueError("conditional_smc: uniforms[{}] must be [{}, {}] float64".format(time, batch_size, columns))
        return u

    try:
        with torch.no_grad(), _syncfree.scope():
            reference = [_lazy.real(x).detach() for x in reference]
            history, log_weights, ancestral = [], [], []
            for time in range(num_timesteps):
                if time == 0:
                    ancestors = None
                    proposal_dist = proposal(time=0, observations=observations)
                else:
                    previous, stored = log_weights[-1], history[-1]
                    u = block(time - 1, previous.device)
                    if ancestor_sampling:
                        distribution = transition(previous_latents=list(history), time=time,
                                                  previous_observations=observations[:time])
                        loc, scale = smoothing._normal_terms(distribution, stored, _refuse)
                        if not provider.conditional_ancestor_index_covers(previous, u, loc, reference[time], scale):
                            _refuse("these log-weights, uniforms, locations and scales together (one dtype, float32 or "
                                    "float64, on one device)")
                        index = provider.conditional_ancestor_index(previous, u, loc, reference[time], scale)
                    else:
                        index = provider.conditional_ancestor_index(previous, u)
                    ancestral.append(index)
                    ancestors = inference.ResampledHistory(history, index)
                    proposal_dist = proposal(previous_latents=ancestors, time=time, observations=observations)
                if isinstance(proposal_dist, dict):
                    _refuse("dict latents")
                latent = state.materialise_draw(state.sample(proposal_dist, batch_size, num_particles))
                if not torch.is_tensor(latent) or latent.dtype not in (torch.float32, torch.float64):
                    _refuse("latents that are no float32 / float64 tensor")
                latent = _lazy.real(latent).detach().contiguous()
                if time == 0:      # every entry of the reference against the latents' shape, before the first resampling
                    for step, x in enumerate(reference):
                        if tuple(x.shape) != (batch_size,) + tuple(latent.shape[2:]) or x.dtype != latent.dtype or \
                                x.device != latent.device:
                            raise ValueError("conditional_smc: reference[{}] must be {} {} on {}, got {} {} on {}".format(
                                step, (batch_size,) + tuple(latent.shape[2:]), latent.dtype, latent.device,
                                tuple(x.shape), x.dtype, x.device))
                latent[:, pinned] = reference[time]
                history.append(latent)
                if time == 0:
                    prior_dist = initial()
                    emission_dist = emission(latents=history, time=0)
                else:
                    prior_dist = transition(previous_latents=ancestors, time=time,
                                            previous_observations=observations[:time])
                    emission_dist = emission(latents=history, time=time, previous_observations=observations[:time])
                log_q = state.log_prob(proposal_dist, latent)
                log_p = state.log_prob(prior_dist, latent)
                log_g = state.log_prob(emission_dist, state.expand_observation(observations[time], num_particles))
                log_weight, _ = _ops.logweight_lse(log_p, log_g, log_q)
                log_weights.append(log_weight)

            device = log_weights[-1].device
            last, _ = provider.backward_sample(log_weights[-1], None, None, None, block(num_timesteps - 1, device))
            indices = [None] * num_timesteps
            indices[-1] = last[:, 0]
            for time in range(num_timesteps - 2, -1, -1):
                # (an index of a flagged row is num_particles: the clamp keeps the read in range, the flag raises below)
                at = indices[time + 1].clamp(max=pinned).unsqueeze(1)
                indices[time] = torch.gather(ancestral[time], 1, at)[:, 0]
            path = []
            for time in range(num_timesteps):
                x = history[time]
                at = indices[time].clamp(max=pinned).reshape((batch_size, 1) + (1,) * (x.dim() - 2))
                path.append(torch.gather(x, 1, at.expand((batch_size, 1) + tuple(x.shape[2:])))[:, 0])
            inference._raise_for_flags(provider.read_flags(device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    if return_particles:
        return path, {"latents": history, "log_weights": log_weights, "ancestral_indices": ancestral, "indices": indices}
    return path


def particle_gibbs(observations, initial, transition, emission, proposal, num_particles, num_sweeps, reference=None,
                   ancestor_sampling=True, burn_in=0):
    """Runs `num_sweeps` sweeps of `conditional_smc`, each from the path the one before returned: batch_size independent
    Markov chains on trajectories whose stationary law is p(x_0..x_{T-1} | y_0..y_{T-1}).

    reference: the first path, T tensors [batch_size, ...]; None — one draw from an ordinary `inference.infer("smc", ...)`
        run with num_particles particles: one categorical draw per row from its final weights, followed back along its
        genealogy.  That run consumes numpy's RandomState as `infer` does (one block of uniforms per resampling step
        under systematic resampling); the sweeps themselves do not — they draw from torch's generator only.
    burn_in: the first `burn_in` sweeps are run and not returned.
    The other arguments are `conditional_smc`'s.

    Returns T tensors [batch_size, num_sweeps - burn_in, ...]: out[t][b, s] is x_t of chain b after sweep burn_in + s.
    Successive sweeps of a chain are dependent draws; the chains are independent of one another."""
    num_sweeps, burn_in = int(num_sweeps), int(burn_in)
    if not 0 <= burn_in < num_sweeps:
        raise ValueError("particle_gibbs: 0 <= burn_in < num_sweeps, got burn_in = {} and num_sweeps = {}".format(
            burn_in, num_sweeps))
    if int(num_particles) > _kernels.HipKernels.CONDITIONAL_MAX_PARTICLES:
        _refuse("num_particles = {}".format(num_particles))
    if reference is None:
        out = inference.infer("smc", observations, initial, transition, emission, proposal, num_particles,
                              return_latents=True, return_log_weight=True)
        if any(isinstance(x, dict) for x in out["latents"]):
            _refuse("dict latents")
        with torch.no_grad():
            log_weight = out["log_weight"].detach()
            batch_size = log_weight.size(0)
            u = torch.rand((batch_size, 1), dtype=torch.float64, device=log_weight.device)
            slot, _ = _kernels.get().backward_sample(log_weight, None, None, None, u)
            reference = []
            for x in out["latents"]:
                x = _lazy.real(x).detach()
                at = slot.clamp(max=x.size(1) - 1).reshape((batch_size, 1) + (1,) * (x.dim() - 2))
                reference.append(torch.gather(x, 1, at.expand((batch_size, 1) + tuple(x.shape[2:])))[:, 0])
            inference.check_device_status(log_weight.device)
    path, kept = list(reference), []
    for sweep in range(num_sweeps):
        path = conditional_smc(observations, initial, transition, emission, proposal, num_particles, path,
                               ancestor_sampling=ancestor_sampling)
        if sweep >= burn_in:
            kept.append(path)
    return [torch.stack([paths[time] for paths in kept], dim=1) for time in range(len(path))]
