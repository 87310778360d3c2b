"""Smoothing from the particles an SMC run has already stored: p(x_0..x_{T-1} | y_0..y_{T-1}) instead of the filter's
p(x_t | y_0..y_t).  Four smoothers, all over `infer(..., return_original_latents=True, return_log_weights=True)`:

`backward_simulate` / `smooth` — forward filtering / backward SIMULATION (FFBS; Godsill, Doucet & West 2004): M equally
    weighted draws from the JOINT smoothing distribution.  O(M K) pairs per step; use it when whole trajectories are
    wanted (functions of several timesteps at once, plots of paths), or when M << K draws are enough.
`marginal_log_weights` / `marginal_smooth` — forward filtering / backward SMOOTHING (FFBSm; Huerzeler & Kuensch 1998;
    Doucet, Godsill & Andrieu 2000): new log-weights for the stored particles of every step, deterministic, so that

        smoothed = smoothing.marginal_log_weights(latents, log_weights, transition, observations)
        mean_t = statistics.empirical_mean(latents[t], smoothed[t])          # E[x_t | y_0..y_{T-1}]

    (likewise `empirical_variance`, `empirical_expectation`, `ess`).  O(K^2) pairs per step, twice; use it for smoothed
    means, variances or any E[f(x_t) | all observations] — no Monte-Carlo noise on top of the filter's.  The cost is
    quadratic in earnest: at B = 1024, K = 4096, T = 100 it is 2 * 99 * 1024 * 4096^2 = 3.4e12 pairs per call — seconds,
    not milliseconds (profiles/ffbsm_pairwise_lse.txt).
`two_slice_expectation` / `two_slice_smooth` — the TWO-SLICE smoother: E[g(x_{t+1}) f(x_t)^T | y_0..y_{T-1}] for every
    pair of neighbouring steps, AND the marginal smoother's weights, from one backward pass.  The lag-one cross moment
    E[x_{t+1} x_t^T] of an EM M-step for the transition, the statistic of a Fisher-identity score, any smoothed additive
    functional (examples/lgssm_em.py).  O(K^2) pairs per step, twice, like the marginal smoother
    (profiles/ffbsm_pairwise_mean.txt).
`map_trajectory` / `map_smooth` — the MAP sequence estimate (Godsill, Doucet & West 2001): the single most probable path
    through the stored particles, argmax over all K^T of them of p(x_0..x_{T-1}, y_0..y_{T-1}), by a Viterbi (max-product)
    recursion, and that path's joint log-density.  Use it when ONE trajectory is wanted that is itself probable — on a
    multimodal posterior the smoothed means are near no probable path, and the best genealogy line or the best of M
    backward-simulated paths searches K or M of the K^T.  It needs the particles only, NO `log_weights`: the filter's
    weights answer "how much mass", this asks "which path", from the model's densities alone.  O(K^2) pairs per step,
    once, deterministic (profiles/map_pairwise_argmax.txt).
`aesmc_amd.particle_gibbs` (another module) — when the particles of ONE filter run are not enough: all four above are only
    as good as the run underneath them, and all but FFBS are quadratic in the particle count.  Particle Gibbs with ancestor
    sampling is a Markov kernel on whole trajectories that leaves the joint smoothing distribution exactly invariant for
    any number of particles; it mixes with K = 8 .. 64, costs O(K) per step and sweep, and is the sampling step of
    parameter learning (particle Gibbs, stochastic-approximation or Monte-Carlo EM).

The smoothed posterior `infer(..., return_latents=True)` gives is the genealogy (`inference.get_resampled_latents`): every
final particle traced back through the ancestor indices.  Over a long sequence the genealogy collapses — after a hundred
resampling steps a thousand final particles descend from a dozen or two particles at time 0.  Backward simulation instead
re-draws, going backwards in time, which stored particle of step t each trajectory passes through, in proportion to

    exp(log_weights[t][b,k]) * transition(x_{t+1} | latents[t][b,k])

so every stored particle of every step can be reached.  The draw is kernel K21 (`aesmc_backward_sample`: a pairwise
trajectory x particle score with one categorical draw per trajectory, O(B M K D) per step, nothing of size [M,K] stored).
The marginal smoother sums where backward simulation draws:

    w[t|T][i] = w[t][i] * sum_j w[t+1|T][j] f(x[t+1][j] | x[t][i]) / (sum_l w[t][l] f(x[t+1][j] | x[t][l]))

two launches of kernel K22 per step (`aesmc_pairwise_lse`: a pairwise particle x particle log-sum-exp, O(B K^2 D), nothing
of size [K,K] stored): the denominators, then the weights.  The two-slice weights fall out of the same recursion:

    W[t][i,j] = w[t][i] f(x[t+1][j] | x[t][i]) w[t+1|T][j] / den[j],       den[j] = sum_l w[t][l] f(x[t+1][j] | x[t][l])
    E[g(x_{t+1}) f(x_t)^T | y] = sum_j w[t+1|T][j] g(x[t+1][j]) m[j]^T
    m[j] = sum_i softmax_i(log w[t][i] + log f(x[t+1][j] | x[t][i])) f(x[t][i])

m[j] is the mean of a payload under the backward kernel of particle j — the pass that forms den[j], carrying a vector per
column: kernel K23 (`aesmc_pairwise_mean`, O(B K^2 (D + P)), nothing of size [K,K] stored) in place of the first of K22's
two launches, den[j] being its normaliser.  The MAP trajectory maximises where the marginal smoother sums:

    delta[t][j] = log g(y_t | x[t][j]) + max_i ( delta[t-1][i] + log f(x[t][j] | x[t-1][i]) )

one launch of kernel K24 per step (`aesmc_pairwise_argmax`: K22's scores, their maximum and its smallest column, O(B K^2 D),
nothing of size [K,K] stored), forwards in time, then a walk back along the stored arguments.

The reference has no counterpart; this module adds to its interface and changes none of it.
"""
import torch

from . import _kernels
from . import _lazy
from . import _syncfree
from . import inference
from . import math
from . import state
from .linear_gaussian import AffineNormal

MAX_LATENT_DIM = 256
_LOG_2PI = 1.8378770664093453      # log(2 pi)
_COVERED = ("covered: a transition that returns an AffineNormal or a torch.distributions.Normal in FULLY_EXPANDED "
            "batch-shape mode, its location shaped like the latent [batch_size, num_particles, ...] with at most {} "
            "values per particle, its scale one value or one per latent dimension (not varying over batch or "
            "particle, by shape or zero strides); tensor latents".format(MAX_LATENT_DIM))


def _refuse(what):
    raise NotImplementedError("aesmc_amd.smoothing: {} is not implemented; {}".format(what, _COVERED))


def _normal_terms(distribution, latent, refuse, what="transition", detach=True):
    """(loc [B,K,...], scale of 1 or D values) of a covered Normal over `latent`'s particles — the recognition this module
    and `aesmc_amd.marginal_filter` share.  `refuse(text)` raises the caller's NotImplementedError; `what` names the
    callable in its text; `detach`: the smoothers post-process, the marginal filter differentiates."""
    if isinstance(distribution, dict):
        refuse("a dict of {} distributions".format(what))
    if type(distribution) not in (AffineNormal, torch.distributions.Normal):
        refuse("a {} distribution of type {}".format(what, type(distribution).__name__))
    loc, scale = distribution.loc, distribution.scale      # (an AffineNormal's location: kernel K8, once)
    batch_size, num_particles = latent.shape[:2]
    if state.get_batch_shape_mode(distribution, batch_size, num_particles) != state.BatchShapeMode.FULLY_EXPANDED:
        refuse("a {} that is not in FULLY_EXPANDED batch-shape mode".format(what))
    loc = _lazy.real(loc)
    loc = loc.detach() if detach else loc
    if tuple(loc.shape) != tuple(latent.shape) or loc.dtype != latent.dtype:
        refuse("a {} location of shape {} {} for latents of shape {} {}".format(
            what, tuple(loc.shape), loc.dtype, tuple(latent.shape), latent.dtype))
    dim = 1
    for size in latent.shape[2:]:
        dim *= size
    if dim > MAX_LATENT_DIM:
        refuse("a latent of {} values per particle (D > {})".format(dim, MAX_LATENT_DIM))
    scale = _lazy.real(scale)
    scale = scale.detach() if detach else scale
    if tuple(scale.shape) != tuple(latent.shape):
        try:
            scale = scale.expand(latent.shape)
        except RuntimeError:
            refuse("a scale of shape {} for latents of shape {}".format(tuple(scale.shape), tuple(latent.shape)))
    if any(size != 1 and stride != 0 for size, stride in zip(scale.shape[:2], scale.stride()[:2])):
        refuse("a scale that varies over batch or particle (a particle-dependent scale)")
    per_dim = scale[0, 0]
    if all(size == 1 or stride == 0 for size, stride in zip(per_dim.shape, per_dim.stride())):
        values = per_dim.reshape(-1)[:1]      # one value for the whole latent
    else:
        values = per_dim.reshape(-1)
    return loc, values.to(latent.dtype)


def _transition_terms(distribution, latent):
    """(loc [B,K,...], scale of 1 or D values) of a covered transition distribution over `latent`'s particles."""
    return _normal_terms(distribution, latent, _refuse)


def backward_simulate(latents, log_weights, transition, num_trajectories=None, observations=None, uniforms=None,
                      return_indices=False):
    """Backward simulation over the particles of one SMC run.

    latents, log_weights: what `infer("smc", ..., return_original_latents=True, return_log_weights=True)` returned as
        `original_latents` and `log_weights` — T tensors [batch_size, num_particles, ...] (the particles as drawn, before
        resampling) and T tensors [batch_size, num_particles].
    transition: the model's transition callable.  For t = T-2 ... 0 it is called ONCE on the stored particles, as
        `transition(previous_latents=latents[:t+1], time=t+1, previous_observations=observations[:t+1])` with plain
        tensors.  MARKOV MODELS ONLY: `previous_latents[-1]` must be all of the latents the transition reads — the
        earlier entries handed over are the filter's stored particles, not the trajectories' own pasts.
    num_trajectories: M, trajectories per batch element (default: num_particles).
    observations: handed to the transition (None: it gets `previous_observations=None`).
    uniforms: None — one `torch.rand((batch_size, M), dtype=torch.float64)` block per timestep on the particles' device,
        from torch's generator for that device, drawn for t = T-1 first and t = 0 last (seed with torch.manual_seed;
        numpy's RandomState is not consumed); or a length-T sequence of such blocks, `uniforms[t]` for the draw at time t
        (replay).  Inside `distributed.shard_scope`, None raises NotImplementedError (as stratified resampling does: the
        device draws have no global block that every rank could cut its rows from).
    return_indices: also return which stored particle each trajectory passes through, T int64 tensors [batch_size, M].

    Returns T tensors [batch_size, M, ...]: trajectory m of batch element b is (out[0][b,m], ..., out[T-1][b,m]), an
    equally weighted draw from the joint smoothing distribution; detached.  With `return_indices`: (trajectories, indices).

    Covered: a transition that returns an `AffineNormal` or a `torch.distributions.Normal` in FULLY_EXPANDED batch-shape
    mode, its location shaped like the latent with at most 256 values per particle (trailing dims are flattened; a
    [batch_size, num_particles] latent has one), its scale one value or one per latent dimension, not varying over batch
    or particle (by shape or zero strides).  Everything else — dict latents, other distributions, a particle-dependent
    scale, more than 256 values — raises NotImplementedError.  NaN log-weights or locations raise FloatingPointError, a
    row without a finite maximum RuntimeError — read once, at the end (one synchronisation per call).  Not capturable
    into a hipGraph."""
    num_timesteps = len(latents)
    if num_timesteps == 0 or len(log_weights) != num_timesteps:
        raise ValueError("backward_simulate: latents and log_weights must be equally long and not empty, got {} and {}"
                         .format(num_timesteps, len(log_weights)))
    if any(isinstance(latent, dict) for latent in latents):
        _refuse("dict latents")
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            latents = [_lazy.real(latent).detach() for latent in latents]
            log_weights = [_lazy.real(log_weight).detach() for log_weight in log_weights]
            batch_size, num_particles = log_weights[-1].shape
            device = log_weights[-1].device
            num_trajectories = num_particles if num_trajectories is None else int(num_trajectories)
            if num_trajectories < 0:
                raise ValueError("backward_simulate: num_trajectories must not be negative")
            if uniforms is None:
                from . import distributed
                if distributed.active_shard() is not None:
                    raise NotImplementedError(
                        "aesmc_amd: backward_simulate inside distributed.shard_scope draws its uniforms on the device, "
                        "where no global block exists that every rank could cut its rows from. Pass uniforms= (one "
                        "[batch_size, num_trajectories] float64 block per timestep).")
            elif len(uniforms) != num_timesteps:
                raise ValueError("backward_simulate: uniforms must hold one block per timestep ({}), got {}".format(
                    num_timesteps, len(uniforms)))

            def block(time):
                if uniforms is None:
                    return torch.rand((batch_size, num_trajectories), dtype=torch.float64, device=device)
                u = uniforms[time]
                if tuple(u.shape) != (batch_size, num_trajectories) or u.dtype != torch.float64:
                    raise ValueError("backward_simulate: uniforms[{}] must be [{}, {}] float64, got {} {}".format(
                        time, batch_size, num_trajectories, tuple(u.shape), u.dtype))
                return u

            trajectories, indices = [None] * num_timesteps, [None] * num_timesteps
            indices[-1], trajectories[-1] = provider.backward_sample(log_weights[-1], None, None, None,
                                                                     block(num_timesteps - 1), payload=latents[-1])
            for time in range(num_timesteps - 2, -1, -1):
                distribution = transition(
                    previous_latents=latents[:time + 1], time=time + 1,
                    previous_observations=None if observations is None else observations[:time + 1])
                loc, scale = _transition_terms(distribution, latents[time])
                indices[time], trajectories[time] = provider.backward_sample(
                    log_weights[time], loc, trajectories[time + 1], scale, block(time), payload=latents[time])
            inference._raise_for_flags(provider.read_flags(device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return (trajectories, indices) if return_indices else trajectories


def smooth(observations, initial, transition, emission, proposal, num_particles, num_trajectories=None, resampling=None):
    """Runs the SMC filter (`inference.infer("smc", ...)`, keeping the particles as drawn and every step's log-weights)
    and then `backward_simulate` over what it stored.  Returns (trajectories, log_marginal_likelihood): T tensors
    [batch_size, num_trajectories, ...] (default: num_particles trajectories) and the filter's [batch_size] estimate."""
    out = inference.infer("smc", observations, initial, transition, emission, proposal, num_particles,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True, resampling=resampling)
    trajectories = backward_simulate(out["original_latents"], out["log_weights"], transition,
                                     num_trajectories=num_trajectories, observations=observations)
    return trajectories, out["log_marginal_likelihood"]


def marginal_log_weights(latents, log_weights, transition, observations=None):
    """The marginal particle smoother (FFBSm) over the particles of one SMC run: the log of the weights w[t|T] that make
    the stored particles of step t a sample of p(x_t | y_0..y_{T-1}).

    latents, log_weights, transition, observations: as `backward_simulate` takes them, with the same contract for the
        transition — for t = T-2 ... 0 it is called ONCE on the stored particles, as `transition(previous_latents=
        latents[:t+1], time=t+1, previous_observations=observations[:t+1])` with plain tensors; MARKOV MODELS ONLY.
        The log-weights need not be normalised.  Latents and log-weights share one dtype (float32 or float64), else
        ValueError; the steps may hold different numbers of particles.

    Returns T tensors [batch_size, num_particles] in `log_weights`' dtype, detached and normalised (every row's
    log-sum-exp is 0 up to rounding): `statistics.empirical_mean(latents[t], out[t])` is the smoothed mean.  The last is
    `math.lognormexp(log_weights[-1], dim=1)`; every earlier step is two launches of kernel K22 — O(batch_size
    num_particles^2) pairs each, in float64 — and nothing else.  Deterministic: no random stream is consumed, and batch
    rows are independent, so it works unchanged inside `distributed.shard_scope`.

    Covered and refused as in `backward_simulate`.  NaN log-weights, particles or locations raise FloatingPointError; a
    particle of step t+1 that no particle of step t can reach (a denominator without mass) RuntimeError — read once, at
    the end (one synchronisation per call).  Not capturable into a hipGraph."""
    num_timesteps = len(latents)
    if num_timesteps == 0 or len(log_weights) != num_timesteps:
        raise ValueError("marginal_log_weights: latents and log_weights must be equally long and not empty, got {} and {}"
                         .format(num_timesteps, len(log_weights)))
    if any(isinstance(latent, dict) for latent in latents):
        _refuse("dict latents")
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            latents = [_lazy.real(latent).detach() for latent in latents]
            log_weights = [_lazy.real(log_weight).detach() for log_weight in log_weights]
            smoothed = [None] * num_timesteps
            smoothed[-1] = math.lognormexp(log_weights[-1], dim=1)
            for time in range(num_timesteps - 2, -1, -1):
                distribution = transition(
                    previous_latents=latents[:time + 1], time=time + 1,
                    previous_observations=None if observations is None else observations[:time + 1])
                loc, scale = _transition_terms(distribution, latents[time])
                following = latents[time + 1]
                denominators = provider.pairwise_lse(following, loc, scale, log_weights[time])
                smoothed[time] = provider.pairwise_lse(loc, following, scale, smoothed[time + 1], col_sub=denominators,
                                                       row_add=log_weights[time])
            inference._raise_for_flags(provider.read_flags(log_weights[-1].device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return smoothed


def marginal_smooth(observations, initial, transition, emission, proposal, num_particles, resampling=None):
    """Runs the SMC filter (`inference.infer("smc", ...)`, keeping the particles as drawn and every step's log-weights)
    and then `marginal_log_weights` over what it stored.  Returns (original_latents, smoothed_log_weights,
    log_marginal_likelihood): T tensors [batch_size, num_particles, ...], T tensors [batch_size, num_particles] and the
    filter's [batch_size] estimate."""
    out = inference.infer("smc", observations, initial, transition, emission, proposal, num_particles,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True, resampling=resampling)
    smoothed = marginal_log_weights(out["original_latents"], out["log_weights"], transition, observations=observations)
    return out["original_latents"], smoothed, out["log_marginal_likelihood"]


def _feature(function, time, latent, limit, what):
    """`function(time, latent)` (None: the latent itself) as a [B,K,n] tensor of the latent's dtype: trailing dims flattened."""
    value = latent if function is None else function(time, latent)
    if not torch.is_tensor(value) or value.dim() < 2 or tuple(value.shape[:2]) != tuple(latent.shape[:2]):
        raise ValueError("two_slice_expectation: {} must return a tensor [batch_size, num_particles, ...], got {}".format(
            what, tuple(value.shape) if torch.is_tensor(value) else type(value).__name__))
    value = _lazy.real(value).detach()
    if value.dtype != latent.dtype or value.device != latent.device:
        raise ValueError("two_slice_expectation: {} must keep the latents' dtype and device, got {} on {}".format(
            what, value.dtype, value.device))
    value = value.reshape(value.shape[0], value.shape[1], -1) if value.dim() != 3 else value
    if limit is not None and not 1 <= value.shape[2] <= limit:
        _refuse("{} of {} values per particle (1 <= P <= {})".format(what, value.shape[2], limit))
    return value


def two_slice_expectation(latents, log_weights, transition, observations=None, previous=None, following=None):
    """The two-slice particle smoother over the particles of one SMC run:

        expectations[t][b,q,p] = E[ following_q(x_{t+1}) previous_p(x_t) | y_0..y_{T-1} ],     t = 0 .. T-2

    and the marginal smoother's log-weights, from ONE backward pass.

    latents, log_weights, transition, observations: as `marginal_log_weights` takes them, with the same contract for the
        transition — for t = T-2 ... 0 it is called ONCE on the stored particles, as `transition(previous_latents=
        latents[:t+1], time=t+1, previous_observations=observations[:t+1])` with plain tensors; MARKOV MODELS ONLY:
        `previous_latents[-1]` must be all of the latents the transition reads.
    previous, following: None — the latent itself, trailing dims flattened; or a callable `(time, latent [batch_size,
        num_particles, ...]) -> tensor [batch_size, num_particles, ...]` in the latents' dtype, flattened to P (at most
        256, else NotImplementedError) and Q (any number of) values.  Per step, each is called once, on plain detached
        tensors: `previous(t, latents[t])` and `following(t + 1, latents[t + 1])`.

    Returns (expectations, smoothed): T-1 tensors [batch_size, Q, P] in the latents' dtype (an empty list for T = 1), and
    T tensors [batch_size, num_particles], exactly what `marginal_log_weights` documents.  With the defaults
    `expectations[t]` is E[x_{t+1} x_t^T | y]; `previous = lambda t, x: x.new_ones(x.shape[0], x.shape[1], 1)` reproduces
    E[following(x_{t+1}) | y] (the marginal means under smoothed[t+1]), `following = ones` likewise E[previous(x_t) | y]
    under smoothed[t].

    Per step: one launch of kernel K23 (the backward kernel's mean m[j] of `previous` for every particle j of step t+1,
    and the denominators), one of K22 (the smoothed log-weights of step t) and the contraction sum_j exp(smoothed[t+1][j])
    following_j (x) m_j as a float64 batched product, rounded once — O(batch_size num_particles^2 (D + P)) per step, in
    float64, nothing of size [num_particles, num_particles] stored.  Deterministic: no random stream is consumed, and
    batch rows are independent, so it works unchanged inside `distributed.shard_scope`.

    Covered and refused as in `backward_simulate`.  NaN log-weights, particles, locations or features raise
    FloatingPointError; a particle of step t+1 that no particle of step t can reach RuntimeError — read once, at the end
    (one synchronisation per call).  Not capturable into a hipGraph."""
    num_timesteps = len(latents)
    if num_timesteps == 0 or len(log_weights) != num_timesteps:
        raise ValueError("two_slice_expectation: latents and log_weights must be equally long and not empty, got {} and {}"
                         .format(num_timesteps, len(log_weights)))
    if any(isinstance(latent, dict) for latent in latents):
        _refuse("dict latents")
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            latents = [_lazy.real(latent).detach() for latent in latents]
            log_weights = [_lazy.real(log_weight).detach() for log_weight in log_weights]
            smoothed = [None] * num_timesteps
            expectations = [None] * (num_timesteps - 1)
            smoothed[-1] = math.lognormexp(log_weights[-1], dim=1)
            for time in range(num_timesteps - 2, -1, -1):
                distribution = transition(
                    previous_latents=latents[:time + 1], time=time + 1,
                    previous_observations=None if observations is None else observations[:time + 1])
                loc, scale = _transition_terms(distribution, latents[time])
                after = latents[time + 1]
                payload = _feature(previous, time, latents[time], _kernels.HipKernels.PAIRWISE_MEAN_MAX_PAYLOAD,
                                   "a `previous` feature")
                outer = _feature(following, time + 1, after, None, "a `following` feature")
                means, denominators = provider.pairwise_mean(after, loc, scale, log_weights[time], payload)
                smoothed[time] = provider.pairwise_lse(loc, after, scale, smoothed[time + 1], col_sub=denominators,
                                                       row_add=log_weights[time])
                weighted = outer.double() * torch.exp(smoothed[time + 1].double()).unsqueeze(-1)
                expectations[time] = torch.bmm(weighted.transpose(1, 2), means.double()).to(after.dtype)
            inference._raise_for_flags(provider.read_flags(log_weights[-1].device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return expectations, smoothed


def two_slice_smooth(observations, initial, transition, emission, proposal, num_particles, resampling=None, previous=None,
                     following=None):
    """Runs the SMC filter (`inference.infer("smc", ...)`, keeping the particles as drawn and every step's log-weights)
    and then `two_slice_expectation` over what it stored.  Returns (original_latents, smoothed_log_weights, expectations,
    log_marginal_likelihood): T tensors [batch_size, num_particles, ...], T tensors [batch_size, num_particles], T-1
    tensors [batch_size, Q, P] and the filter's [batch_size] estimate."""
    out = inference.infer("smc", observations, initial, transition, emission, proposal, num_particles,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True, resampling=resampling)
    expectations, smoothed = two_slice_expectation(out["original_latents"], out["log_weights"], transition,
                                                   observations=observations, previous=previous, following=following)
    return out["original_latents"], smoothed, expectations, out["log_marginal_likelihood"]


def map_trajectory(latents, initial, transition, emission, observations, return_indices=False):
    """The MAP sequence estimate over the particles of one SMC run (the particle Viterbi recursion of Godsill, Doucet &
    West 2001): of all K^T paths through the stored particles, the one of largest joint density p(x_0..x_{T-1},
    y_0..y_{T-1}).

    latents: what `infer("smc", ..., return_original_latents=True)` returned as `original_latents` — T tensors
        [batch_size, num_particles, ...] (the particles as drawn, before resampling); the steps may hold different
        numbers of particles.  No log-weights are needed.
    initial, transition, emission: the model's callables, each called ONCE per step on plain detached tensors, forwards
        in time: `initial()` once; `emission(latents=latents[:t+1], time=t, previous_observations=observations[:t])` for
        t = 0 ... T-1, without the `previous_observations` keyword at t = 0 — exactly how `infer` calls it; and
        `transition(previous_latents=latents[:t+1], time=t+1, previous_observations=observations[:t+1])` for t = 0 ...
        T-2, as the other smoothers call it.  MARKOV MODELS ONLY: `previous_latents[-1]` must be all of the latents the
        transition reads, and `latents[-1]` all the emission reads.
    observations: length-T sequence of [batch_size, ...] tensors.
    return_indices: also return which stored particle the path passes through, T int64 tensors [batch_size].

    Returns (trajectory, log_joint): T tensors [batch_size, ...] gathered from `latents` (the stored values exactly,
    detached), and [batch_size] in the latents' dtype, log p(x*_{0..T-1}, y_{0..T-1}) of that path with the transition's
    normalising constant included.  With `return_indices`: (trajectory, log_joint, indices).  Ties go to the smallest
    particle index.

    The transition is covered and refused as in `backward_simulate`.  The initial and emission log-densities go through
    `state.log_prob` (with `state.expand_observation`), O(batch_size num_particles) per step: any distribution
    `state.log_prob` takes is covered, the emission need not be Normal.  The recursion is carried in FLOAT64 whatever the
    latents' dtype (the per-step operands are upcast: O(batch_size num_particles D) memory beside O(batch_size
    num_particles^2 D) work) — with float32 deltas the rounding would be of the size of real gaps between candidate paths,
    and the path would depend on it.  T - 1 launches of kernel K24, one more without a distance term for the final
    maximum, T - 1 gathers for the walk back.  Deterministic: no random stream is consumed, and batch rows are
    independent, so it works unchanged inside `distributed.shard_scope`.

    NaN densities, particles or locations raise FloatingPointError, a density of +inf RuntimeError, a batch row whose
    best path has log_joint == -inf (no path of positive density) RuntimeError — read once, at the end (one
    synchronisation per call).  Not capturable into a hipGraph."""
    num_timesteps = len(latents)
    if num_timesteps == 0 or len(observations) != num_timesteps:
        raise ValueError("map_trajectory: latents and observations must be equally long and not empty, got {} and {}"
                         .format(num_timesteps, len(observations)))
    if any(isinstance(latent, dict) for latent in latents):
        _refuse("dict latents")
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            latents = [_lazy.real(latent).detach() for latent in latents]
            first = latents[0]
            batch_size, dtype, wide = first.shape[0], first.dtype, torch.float64

            def density(distribution, value, num_particles):      # [batch_size, num_particles] float64
                return _lazy.real(state.log_prob(distribution, value)).detach().expand(batch_size, num_particles).to(wide)

            def emission_term(time):
                history = latents[:time + 1]
                if time == 0:
                    distribution = emission(latents=history, time=0)
                else:
                    distribution = emission(latents=history, time=time, previous_observations=observations[:time])
                num_particles = latents[time].shape[1]
                return density(distribution, state.expand_observation(observations[time], num_particles), num_particles)

            delta = density(initial(), first, first.shape[1]) + emission_term(0)
            arguments = [None] * num_timesteps
            for time in range(1, num_timesteps):
                distribution = transition(previous_latents=latents[:time], time=time,
                                          previous_observations=observations[:time])
                loc, scale = _transition_terms(distribution, latents[time - 1])
                current = latents[time]
                if current.dim() != loc.dim() or tuple(current.shape[2:]) != tuple(loc.shape[2:]) or \
                        current.dtype != dtype:
                    _refuse("latents of shape {} {} after latents of shape {} {}".format(
                        tuple(current.shape), current.dtype, tuple(loc.shape), dtype))
                dim = 1
                for size in current.shape[2:]:
                    dim *= size
                scale = scale.to(wide)
                # the transition's normalising constant: - sum_d log scale[d] - D/2 log(2 pi), a 0-dim tensor
                constant = -(torch.log(scale).sum() * (dim // scale.numel())) - 0.5 * dim * _LOG_2PI
                delta, arguments[time] = provider.pairwise_argmax(current.to(wide), loc.to(wide), scale, delta,
                                                                  row_add=emission_term(time) + constant)
            nothing = delta.new_empty((batch_size, 1, 0))
            best, last = provider.pairwise_argmax(nothing, delta.new_empty(delta.shape + (0,)), None, delta)
            log_joint = best[:, 0]
            rows = torch.arange(batch_size, device=delta.device)
            indices, trajectory = [None] * num_timesteps, [None] * num_timesteps
            index = last[:, 0].clamp(max=delta.shape[1] - 1)      # ("no column" is clamped, never dereferenced)
            for time in range(num_timesteps - 1, -1, -1):
                indices[time], trajectory[time] = index, latents[time][rows, index]
                if time > 0:
                    index = arguments[time].gather(1, index.unsqueeze(1)).squeeze(1).clamp(max=latents[time - 1].shape[1] - 1)
            inference._raise_for_flags(provider.read_flags(delta.device))
            if bool((log_joint == -float("inf")).any()):          # (after the one synchronisation: nothing is pending)
                raise RuntimeError("map_trajectory: no path of positive density through the stored particles (log_joint "
                                   "== -inf) in batch row(s) {}".format(
                                       torch.nonzero(log_joint == -float("inf")).reshape(-1).tolist()))
    except BaseException:
        inference._discard_pending_flags()
        raise
    log_joint = log_joint.to(dtype)
    return (trajectory, log_joint, indices) if return_indices else (trajectory, log_joint)


def map_smooth(observations, initial, transition, emission, proposal, num_particles, resampling=None):
    """Runs the SMC filter (`inference.infer("smc", ...)` with the other smoothers' settings, keeping the particles as
    drawn) and then `map_trajectory` over what it stored.  Returns (trajectory, log_joint, log_marginal_likelihood): T
    tensors [batch_size, ...], the path's joint log-density [batch_size] and the filter's [batch_size] estimate."""
    out = inference.infer("smc", observations, initial, transition, emission, proposal, num_particles,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True, resampling=resampling)
    trajectory, log_joint = map_trajectory(out["original_latents"], initial, transition, emission, observations)
    return trajectory, log_joint, out["log_marginal_likelihood"]
