"""The fully adapted auxiliary particle filter (Pitt & Shephard 1999): the best one-step filter for models whose
transition is Normal with a constant diagonal scale and whose emission is linear-Gaussian in the newest latent,

    x_t ~ N(mu(x_{t-1}), S_f),  S_f = diag(s_f^2)            y_t ~ N(C x_t + d, S_g),  S_g = diag(s_g^2)

— `testing.models.LgssmNd` and `testing.models.NonlinearSsm` (mu = tanh(A x)) are both of that class.  Every other filter
of this package proposes from a q, then weighs: it learns about y_t only after the particles were resampled and moved.
For this class the two quantities an SMC step wants are known in closed form,

    p(y_t | x_{t-1})       = N(y_t; C mu + d, S),                S = C S_f C^T + S_g
    p(x_t | x_{t-1}, y_t)  = N(mu + G (y_t - d - C mu), Sigma),  G = S_f C^T S^-1,  Sigma = S_f - G C S_f

and the adapted filter uses them exactly: it RESAMPLES on p(y_t | x_{t-1}^k), before moving; it DRAWS x_t from the optimal
proposal with its full covariance; and it is left with exactly uniform weights.  `adapted_filter` takes no proposal.

What it is for: a ceiling for a learned proposal (ELBO(learned q) <= ELBO(adapted) <= log p(y), the Kalman filter's); a
much better particle system to hand to `smoothing.backward_simulate`, `marginal_log_weights`, `two_slice_expectation` and
`map_trajectory`, which take its `original_latents` and `log_weights` unchanged; and evidence estimates with a fraction
of the bootstrap filter's variance (a hundredth and less: profiles/adapted_filter.txt).

A step is three launches: K27 (`aesmc_affine_quadratic_logweight`: log lambda = base - 1/2 |P mu + o|^2), the existing
resampling launch K2 on log lambda (its row log-sum-exp is the step's evidence increment), and K28 (`aesmc_adapted_draw`:
x_t = r + M mu[a] + L eps), with the small float64 operands of `gains` formed on the host once per distinct model.

The reference has no counterpart; this module adds to its interface and changes none of it.
"""
import math

import torch

from . import _kernels
from . import _lazy
from . import _ops
from . import _syncfree
from . import inference
from . import linear_gaussian
from . import smoothing
from . import state

MAX_DIM = _kernels.HipKernels.ADAPTED_MAX_DIM
_LOG_2PI = 1.8378770664093453      # log(2 pi)
_COVERED = ("covered: Markov models with tensor latents [batch_size, num_particles, D] and observations [batch_size, Dy] "
            "of float32 or float64, D and Dy at most {0}; an initial() that returns a torch.distributions.Normal with loc "
            "[D] or [batch_size, D] and a scale of one value or D values; a transition that returns an AffineNormal or a "
            "torch.distributions.Normal in FULLY_EXPANDED batch-shape mode, its location shaped like the latent, its "
            "scale one value or one per latent dimension (not varying over batch or particle); an emission that is "
            "linear in the newest latent — an AffineNormal of latents[-1], or Normal(latents[-1] @ C.t() + d, s) — with a "
            "weight [Dy, D], an offset None, [Dy] or [batch_size, Dy] and a scale of one value or Dy values (not varying "
            "over batch or particle)".format(MAX_DIM))


def _refuse(what):
    raise NotImplementedError("aesmc_amd.adapted: {} is not implemented; {}".format(what, _COVERED))


def gains(transition_scale, weight, emission_scale):
    """The float64 operands of an adapted step for one (s_f, C, s_g), by torch.linalg on `weight`'s device:

        S    = C S_f C^T + S_g           chol(S) = Lam Lam^T         W = Lam^-1                          [Dy,Dy]
        G    = S_f C^T S^-1              Sigma = S_f - G C S_f       chol(Sigma) = L L^T                 [D,Dy], [D,D]
        P    = -W C   [Dy,D]             M = I - G C   [D,D]         base = -1/2 Dy log 2 pi - sum_j log Lam_jj

    transition_scale: a tensor of one value or D values; weight: C [Dy,D]; emission_scale: one value or Dy values.
    Returns a dict with P, M, L, W, G (float64 tensors) and base (a Python float).  One host synchronisation.  ValueError
    naming the covariance whose Cholesky factorisation fails."""
    gain, _ = _gain_algebra(transition_scale.detach(), weight.detach(), emission_scale.detach())
    return gain


def differentiable_gains(transition_scale, weight, emission_scale):
    """`gains` with the algebra left on the autograd tape: P, M, L, W, G and `base` (here a 0-dim float64 TENSOR) are
    differentiable functions of the three operands, and `base_value` is base's value as a Python float (what the forward
    launch takes).  The same numbers as `gains`, the same one host synchronisation, the same ValueErrors."""
    gain, log_det = _gain_algebra(transition_scale, weight, emission_scale)
    gain["base_value"] = gain["base"]
    gain["base"] = -0.5 * weight.size(0) * _LOG_2PI - log_det
    return gain


def _gain_algebra(transition_scale, weight, emission_scale):
    """(`gains`' dict, log det chol(S) as a 0-dim tensor) by torch.linalg on whatever tape the operands are on."""
    C = weight.to(torch.float64)
    Dy, D = C.shape

    def variance(scale, size, what):
        scale = scale.to(device=C.device, dtype=torch.float64).reshape(-1)
        if scale.numel() not in (1, size):
            raise ValueError("aesmc_amd.adapted: {} has {} values for {} dimensions".format(what, scale.numel(), size))
        return (scale * scale).expand(size)

    var_f = variance(transition_scale, D, "the transition's scale")
    var_g = variance(emission_scale, Dy, "the emission's scale")
    S = (C * var_f) @ C.t() + torch.diag(var_g)
    lam, bad_s = torch.linalg.cholesky_ex(S)
    W = torch.linalg.solve_triangular(lam, torch.eye(Dy, dtype=torch.float64, device=C.device), upper=False)
    G = (var_f.unsqueeze(1) * C.t()) @ (W.t() @ W)
    sigma = torch.diag(var_f) - G @ (C * var_f)
    L, bad_sigma = torch.linalg.cholesky_ex(0.5 * (sigma + sigma.t()))
    log_det_tensor = torch.log(torch.diagonal(lam)).sum()
    bad_s, bad_sigma, log_det = torch.stack([bad_s.to(torch.float64), bad_sigma.to(torch.float64),
                                             log_det_tensor.detach()]).tolist()
    if bad_s:
        raise ValueError("aesmc_amd.adapted: the Cholesky factorisation of the predictive covariance S = C S_f C^T + S_g "
                         "failed (not positive definite: check the emission's and the transition's scales)")
    if bad_sigma:
        raise ValueError("aesmc_amd.adapted: the Cholesky factorisation of the optimal proposal's covariance Sigma = S_f - "
                         "G C S_f failed (not positive definite: check the transition's scale)")
    gain = {"P": -(W @ C), "M": torch.eye(D, dtype=torch.float64, device=C.device) - G @ C, "L": L.contiguous(), "W": W,
            "G": G, "base": -0.5 * Dy * _LOG_2PI - log_det}
    return gain, log_det_tensor


def _key(tensor):
    return (tensor.data_ptr(), tuple(tensor.shape), tuple(tensor.stride()), tensor.dtype, tensor._version)


class _GainCache:
    """`gains` once per distinct (transition scale, weight, emission scale) for the duration of one call: recognised by
    the tensors' identity (storage, geometry) and `_version`, which are kept alive with the entry."""

    def __init__(self, differentiable=False):
        self._held = {}
        self._differentiable = differentiable      # `differentiable_gains`: the entry carries the call's autograd graph

    def get(self, transition_scale, weight, emission_scale):
        key = (_key(transition_scale), _key(weight), _key(emission_scale))
        entry = self._held.get(key)
        if entry is None:
            form = differentiable_gains if self._differentiable else gains
            entry = self._held[key] = (form(transition_scale, weight, emission_scale),
                                       (transition_scale, weight, emission_scale))
        return entry[0]


def _scale_values(scale, size, what, detach=True):
    """One value or `size` values of a scale that does not vary over anything but its last dimension (`detach` false:
    still on the autograd tape)."""
    scale = _lazy.real(scale)
    scale = scale.detach() if detach else scale
    if scale.numel() == 1:
        return scale.reshape(1)
    if scale.dim() == 0 or scale.size(-1) not in (1, size):
        _refuse("{} of shape {}".format(what, tuple(scale.shape)))
    if any(extent != 1 and stride != 0 for extent, stride in zip(scale.shape[:-1], scale.stride()[:-1])):
        _refuse("{} that varies over batch or particle".format(what))
    values = scale[(0,) * (scale.dim() - 1)]
    return values[:1] if (values.numel() == 1 or values.stride(0) == 0) else values


def _initial_terms(distribution, batch_size, detach=True):
    if type(distribution) is not torch.distributions.Normal:
        _refuse("an initial distribution of type {}".format(type(distribution).__name__))
    loc = _lazy.real(distribution.loc)
    loc = loc.detach() if detach else loc
    if loc.dtype not in (torch.float32, torch.float64):
        _refuse("latents of dtype {}".format(loc.dtype))
    if loc.dim() not in (1, 2) or (loc.dim() == 2 and loc.size(0) != batch_size):
        _refuse("an initial location of shape {}".format(tuple(loc.shape)))
    dim = loc.size(-1)
    if not 1 <= dim <= MAX_DIM:
        _refuse("a latent of {} values per particle (D > {})".format(dim, MAX_DIM))
    return loc.expand(batch_size, dim), _scale_values(distribution.scale, dim, "an initial scale", detach)


def _emission_terms(distribution, stand_in, observation, detach=True):
    """(weight [Dy,D], offset None | [Dy] | [B,Dy], scale of 1 or Dy values) of an emission that is linear in `stand_in`."""
    if isinstance(distribution, dict):
        _refuse("a dict of emission distributions")
    terms = linear_gaussian.affine_terms(distribution)
    if terms is None:
        _refuse("an emission that is not linear-Gaussian in the newest latent ({})".format(type(distribution).__name__))
    if terms.source is not stand_in:
        _refuse("an emission whose location is a map of something other than latents[-1]")
    weight, offset = terms.weight, terms.offset
    batch_size, dim = stand_in.shape[0], stand_in.shape[2]
    if weight.dim() != 2 or weight.size(1) != dim or tuple(observation.shape) != (batch_size, weight.size(0)):
        _refuse("an emission weight of shape {} for latents of {} values and observations of shape {}".format(
            tuple(weight.shape), dim, tuple(observation.shape)))
    if not 1 <= weight.size(0) <= MAX_DIM:
        _refuse("an observation of {} values (Dy > {})".format(weight.size(0), MAX_DIM))
    if offset is not None and tuple(offset.shape) not in ((weight.size(0),), (batch_size, weight.size(0))):
        _refuse("an emission offset of shape {}".format(tuple(offset.shape)))
    return weight, offset, _scale_values(terms.scale_param, weight.size(0), "an emission scale", detach)


def _row_offsets(gain, observation, offset, detach=True):
    """(o [B,Dy], r [B,D]) float64: W (y - d) and G (y - d); `detach` false: differentiable in d and the gains."""
    residual = observation.detach().to(torch.float64)
    if offset is not None:
        residual = residual - (offset.detach() if detach else offset).to(torch.float64)
    return residual @ gain["W"].t(), residual @ gain["G"].t()


def adapted_filter(observations, initial, transition, emission, num_particles, resampling=None, noise=None,
                   return_latents=False, return_first_stage=False):
    """Runs the fully adapted auxiliary particle filter.  It takes no proposal: that is the point.

    observations: length-T sequence of [batch_size, Dy] tensors.
    initial(): a torch.distributions.Normal with loc [D] or [batch_size, D] and a scale of one value or D values.
    transition: called once per step t >= 1 on the STORED (un-resampled) particles, with plain tensors, as
        `transition(previous_latents=originals[:t], time=t, previous_observations=observations[:t])`.  MARKOV MODELS ONLY:
        `previous_latents[-1]` must be all of the latents it reads.  Covered as in `smoothing.backward_simulate`.
    emission: called once per step as `emission(latents=originals[:t] + [mu], time=t, previous_observations=
        observations[:t])` (time 0: no previous_observations) with the transition's LOCATION mu standing in as the newest
        latent (time 0: the initial location, expanded).  It must be linear in it: an `AffineNormal(latents[-1], C, s,
        offset=d)` or `Normal(latents[-1] @ C.t() + d, s)`.  Only its weight, offset and scale are read.
    num_particles: K.
    resampling: 'systematic', 'stratified' or None (`settings.current().resampling`), as `infer` — the uniforms come from
        the same feeds (`uniform_feed(...)` overrides them), and 'stratified' inside `distributed.shard_scope` raises.
    noise: None — the standard-normal draws come from torch's generator on the device (seed with torch.manual_seed); or
        a length-T sequence of [batch_size, num_particles, D] tensors in the latents' dtype (replay).
    return_latents: also trace the genealogy (`inference.get_resampled_latents`).
    return_first_stage: also return the first-stage log-weights.

    Returns a dict with `infer`'s keys: log_marginal_likelihood [batch_size] float64 (unbiased for p(y_0..y_{T-1}); exact for
    T = 1), original_latents (T tensors [batch_size, num_particles, D]), log_weights (T tensors of zeros [batch_size,
    num_particles]: the particles are equally weighted, and the smoothers take this as it is), log_weight (the last of
    them), ancestral_indices (T-1 int64 [batch_size, num_particles], `infer`'s convention: the ancestors of step t+1
    among step t's particles), last_latent, latents (the genealogy or None) and first_stage_log_weights (T-1 tensors
    [batch_size, num_particles]: log p(y_{t+1} | x_t^k) over step t's particles, or None).

    The gain algebra is float64 on the host side of the device (`gains`): once per distinct (transition scale, emission
    weight, emission scale) — a time-invariant model pays once for step 0 (whose "transition scale" is the initial's) and
    once for all later steps, one host synchronisation each; a time-varying one pays per step.

    Anything not covered raises NotImplementedError before the step's launches; a covariance without a Cholesky factor
    ValueError.  NaN locations raise FloatingPointError, a row without a finite maximum RuntimeError — read once, at the
    end; an exception on the way discards whatever was flagged.  Runs under torch.no_grad(): NOT differentiable, and
    (the host reads the gains back) NOT capturable into a hipGraph."""
    num_timesteps, num_particles = len(observations), int(num_particles)
    if num_timesteps == 0:
        raise ValueError("adapted_filter: observations must hold at least one timestep")
    if num_particles < 1:
        raise ValueError("adapted_filter: num_particles must be at least 1")
    if any(isinstance(y, dict) for y in observations):
        _refuse("dict latents or observations")
    if noise is not None and len(noise) != num_timesteps:
        raise ValueError("adapted_filter: noise must hold one tensor per timestep ({}), got {}".format(
            num_timesteps, len(noise)))
    stratified = inference._resolve_resampling(resampling) == "stratified"
    batch_size = observations[0].size(0)
    provider = _kernels.get()
    cache = _GainCache()
    try:
        with torch.no_grad(), _syncfree.scope():
            prior = initial()
            if isinstance(prior, dict):
                _refuse("dict latents or observations")
            loc0, scale0 = _initial_terms(prior, batch_size)
            dtype, device, dim = loc0.dtype, loc0.device, loc0.size(1)
            shape = (batch_size, num_particles, dim)

            def draw(time):
                if noise is None:
                    return state._standard_normal(shape, dtype, device)
                eps = noise[time]
                if not torch.is_tensor(eps) or tuple(eps.shape) != shape or eps.dtype != dtype or eps.device != device:
                    raise ValueError("adapted_filter: noise[{}] must be {} {} on {}".format(time, shape, dtype, device))
                return eps

            def linear_emission(time, mu):
                stand_in = _lazy.LazyGiven(mu)
                if time == 0:
                    distribution = emission(latents=[stand_in], time=0)
                else:
                    distribution = emission(latents=originals + [stand_in], time=time,
                                            previous_observations=observations[:time])
                y = observations[time]
                if not torch.is_tensor(y) or y.dim() != 2:
                    _refuse("observations that are not [batch_size, Dy] tensors")
                return _emission_terms(distribution, stand_in, y)

            # ---- step 0: the same algebra with S_f := diag(scale0^2) and mu := loc0, no particle dependence ------------
            mu = loc0.unsqueeze(1).expand(shape)
            weight, offset, scale_g = linear_emission(0, mu)
            if not provider.adapted_covers(mu, dim, weight.size(0)):
                _refuse("these locations (float32 or float64 [batch_size, num_particles, D] on the HIP device)")
            gain = cache.get(scale0, weight, scale_g)
            o, r = _row_offsets(gain, observations[0], offset)
            residual = loc0.to(torch.float64) @ gain["P"].t() + o
            log_z = gain["base"] - 0.5 * (residual * residual).sum(dim=1)      # log p(y_0), exact
            originals = [provider.adapted_draw(mu, None, gain["M"], r, gain["L"], draw(0))]
            ancestral, first_stage = [], []
            feed = None
            for time in range(1, num_timesteps):
                stored = originals[-1]
                distribution = transition(previous_latents=list(originals), time=time,
                                          previous_observations=observations[:time])
                mu, scale_f = smoothing._normal_terms(distribution, stored, _refuse)
                weight, offset, scale_g = linear_emission(time, mu)
                if not provider.adapted_covers(mu, dim, weight.size(0)):
                    _refuse("these locations (float32 or float64 [batch_size, num_particles, D] on the HIP device)")
                gain = cache.get(scale_f, weight, scale_g)
                o, r = _row_offsets(gain, observations[time], offset)
                log_lambda = provider.affine_quadratic_logweight(mu, gain["P"], o, gain["base"])
                if feed is None:
                    feed = inference._FEED_OVERRIDE.get() or (
                        inference._StratifiedFeed(batch_size, num_particles, device) if stratified else
                        inference._UniformFeed(batch_size, num_timesteps - 1, device))
                uniforms = feed.next()
                per_particle = uniforms.dim() == 2 and tuple(uniforms.shape) == (batch_size, num_particles)
                if per_particle != stratified and num_particles != 1:
                    raise ValueError("aesmc_amd: {} resampling takes {} uniforms per step, the feed returned {}".format(
                        "stratified" if stratified else "systematic",
                        "[batch_size, num_particles]" if stratified else "[batch_size]", tuple(uniforms.shape)))
                index, lse, _ = _ops.resample_step(log_lambda, uniforms, None, want_lse=True)
                index = _kernels.as_index(index)
                log_z = log_z + (lse.to(torch.float64) - math.log(num_particles))
                originals.append(provider.adapted_draw(mu, index, gain["M"], r, gain["L"], draw(time)))
                ancestral.append(index)
                first_stage.append(log_lambda)
            log_weights = [torch.zeros((batch_size, num_particles), dtype=dtype, device=device)
                           for _ in range(num_timesteps)]
            latents = inference.get_resampled_latents(originals, ancestral) if return_latents else None
            inference._raise_for_flags(provider.read_flags(device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return {"log_marginal_likelihood": log_z, "latents": latents, "original_latents": originals,
            "log_weight": log_weights[-1], "log_weights": log_weights, "ancestral_indices": ancestral,
            "last_latent": originals[-1],
            "first_stage_log_weights": first_stage if return_first_stage else None}


def adapted_elbo(observations, initial, transition, emission, num_particles, resampling=None, noise=None):
    """`adapted_filter` with autograd enabled: the same filter for the same covered class, with the same refusals, the
    same uniform and noise feeds and the same numbers — and a `log_marginal_likelihood` [batch_size] float64 that carries
    the graph, so that the model's own parameters (transition map, emission weight and offset, the scales, the initial
    law) can be learned by ascending it.  No proposal is learned: there is none.

    Arguments as `adapted_filter`'s (without its two `return_*` switches); returns its dict without `latents` and
    `first_stage_log_weights`.

    What the gradient is.  The ancestors are HELD FIXED: the indices the resampling launches draw carry no gradient, and
    there is no score-function term for the resampling — what the reference's `infer` (aesmc/inference.py:254) and this
    package's `infer` do as well.  The gradient is therefore that of log Z-hat along the realised genealogy, a BIASED
    estimator of the gradient of E[log Z-hat] (low variance; exact for T <= 2, where no resampling lies on the gradient's
    path).  Everything else is on the tape: the gains P, M, L, W, G and base as float64 functions of the transition's
    scale, the emission's weight and the emission's scale (`differentiable_gains`), the row offsets o = (y - d) W^T and
    r = (y - d) G^T, the exact log p(y_0), the transition's location (`smoothing._normal_terms(..., detach=False)`) of
    the stored particles — the outputs of the previous step's draw, which gives backpropagation through time along the
    genealogy — and step 0's expanded initial location.  K27's adjoint is kernel K29, K28's kernel K30 followed by the
    sorted segmented sum over equal ancestors; the row log-sum-exp differentiates as in `infer`.  First order only.

    Raises NotImplementedError during a hipGraph capture (the host reads the gains back) and inside
    `distributed.shard_scope`; otherwise as `adapted_filter`."""
    from . import distributed
    num_timesteps, num_particles = len(observations), int(num_particles)
    if num_timesteps == 0:
        raise ValueError("adapted_elbo: observations must hold at least one timestep")
    if num_particles < 1:
        raise ValueError("adapted_elbo: num_particles must be at least 1")
    if any(isinstance(y, dict) for y in observations):
        _refuse("dict latents or observations")
    if noise is not None and len(noise) != num_timesteps:
        raise ValueError("adapted_elbo: noise must hold one tensor per timestep ({}), got {}".format(
            num_timesteps, len(noise)))
    if distributed.active_shard() is not None:
        raise NotImplementedError("aesmc_amd.adapted: adapted_elbo inside distributed.shard_scope is not implemented")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise NotImplementedError("aesmc_amd.adapted: adapted_elbo cannot be captured into a hipGraph (the host reads the "
                                  "gains back)")
    stratified = inference._resolve_resampling(resampling) == "stratified"
    batch_size = observations[0].size(0)
    provider = _kernels.get()
    cache = _GainCache(differentiable=True)
    try:
        with torch.enable_grad(), _syncfree.scope():
            prior = initial()
            if isinstance(prior, dict):
                _refuse("dict latents or observations")
            loc0, scale0 = _initial_terms(prior, batch_size, detach=False)
            dtype, device, dim = loc0.dtype, loc0.device, loc0.size(1)
            shape = (batch_size, num_particles, dim)

            def draw(time):
                if noise is None:
                    return state._standard_normal(shape, dtype, device)
                eps = noise[time]
                if not torch.is_tensor(eps) or tuple(eps.shape) != shape or eps.dtype != dtype or eps.device != device:
                    raise ValueError("adapted_elbo: noise[{}] must be {} {} on {}".format(time, shape, dtype, device))
                return eps.detach()

            def linear_emission(time, mu):
                stand_in = _lazy.LazyGiven(mu)
                if time == 0:
                    distribution = emission(latents=[stand_in], time=0)
                else:
                    distribution = emission(latents=originals + [stand_in], time=time,
                                            previous_observations=observations[:time])
                y = observations[time]
                if not torch.is_tensor(y) or y.dim() != 2:
                    _refuse("observations that are not [batch_size, Dy] tensors")
                return _emission_terms(distribution, stand_in, y, detach=False)

            mu = loc0.unsqueeze(1).expand(shape)
            weight, offset, scale_g = linear_emission(0, mu)
            if not provider.adapted_covers(mu, dim, weight.size(0)):
                _refuse("these locations (float32 or float64 [batch_size, num_particles, D] on the HIP device)")
            gain = cache.get(scale0, weight, scale_g)
            o, r = _row_offsets(gain, observations[0], offset, detach=False)
            residual = loc0.to(torch.float64) @ gain["P"].t() + o
            log_z = gain["base"] - 0.5 * (residual * residual).sum(dim=1)      # log p(y_0), exact
            originals = [_ops.adapted_draw(mu, None, gain["M"], r, gain["L"], draw(0))]
            ancestral = []
            feed = None
            for time in range(1, num_timesteps):
                stored = originals[-1]
                distribution = transition(previous_latents=list(originals), time=time,
                                          previous_observations=observations[:time])
                mu, scale_f = smoothing._normal_terms(distribution, stored, _refuse, detach=False)
                weight, offset, scale_g = linear_emission(time, mu)
                if not provider.adapted_covers(mu, dim, weight.size(0)):
                    _refuse("these locations (float32 or float64 [batch_size, num_particles, D] on the HIP device)")
                gain = cache.get(scale_f, weight, scale_g)
                o, r = _row_offsets(gain, observations[time], offset, detach=False)
                log_lambda = _ops.affine_quadratic_logweight(mu, gain["P"], o, gain["base"], gain["base_value"])
                if feed is None:
                    feed = inference._FEED_OVERRIDE.get() or (
                        inference._StratifiedFeed(batch_size, num_particles, device) if stratified else
                        inference._UniformFeed(batch_size, num_timesteps - 1, device))
                uniforms = feed.next()
                per_particle = uniforms.dim() == 2 and tuple(uniforms.shape) == (batch_size, num_particles)
                if per_particle != stratified and num_particles != 1:
                    raise ValueError("aesmc_amd: {} resampling takes {} uniforms per step, the feed returned {}".format(
                        "stratified" if stratified else "systematic",
                        "[batch_size, num_particles]" if stratified else "[batch_size]", tuple(uniforms.shape)))
                index, lse, _ = _ops.resample_step(log_lambda, uniforms, None, want_lse=True)
                index = _kernels.as_index(index)
                log_z = log_z + (lse.to(torch.float64) - math.log(num_particles))
                originals.append(_ops.adapted_draw(mu, index, gain["M"], r, gain["L"], draw(time)))
                ancestral.append(index)
            log_weights = [torch.zeros((batch_size, num_particles), dtype=dtype, device=device)
                           for _ in range(num_timesteps)]
            inference._raise_for_flags(provider.read_flags(device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return {"log_marginal_likelihood": log_z, "original_latents": originals, "log_weight": log_weights[-1],
            "log_weights": log_weights, "ancestral_indices": ancestral, "last_latent": originals[-1]}


def adapted_loss(observations, initial, transition, emission, num_particles, resampling=None, noise=None):
    """Minus the batch mean of `adapted_elbo`'s log_marginal_likelihood: what an optimiser of the model's parameters
    descends.  Arguments as `adapted_elbo`'s."""
    return -adapted_elbo(observations, initial, transition, emission, num_particles, resampling=resampling,
                         noise=noise)["log_marginal_likelihood"].mean()
