"""The Rao-Blackwellised particle filter (mixture Kalman filter; Doucet, de Freitas, Murphy & Russell 2000; Chen & Liu
2000) for switching linear-Gaussian state-space models (SLDS, jump-Markov linear systems):

    s_0 ~ Cat(pi0)                      s_t | s_{t-1} ~ Cat(Pi[s_{t-1}, :])
    z_0 ~ N(m0, diag(s0^2))             z_t = A[s_t] z_{t-1} + b[s_t] + N(0, diag(q[s_t]^2))
    y_t = C[s_t] z_t + d[s_t] + N(0, diag(r[s_t]^2))        (also at t = 0, under s_0)

Every other filter of this package represents the whole latent by samples.  Here only the discrete regime s_t is sampled
(a bootstrap on the regimes); each particle carries the EXACT Kalman mean and covariance of the continuous state z_t given
its regime history, and its weight is the Kalman predictive likelihood p(y_t | s_{0:t}, y_{0:t-1}).  With one regime
(M = 1) the filter is the Kalman filter, exact for any number of particles: `kalman_log_likelihood` is the log p(y) that
`adapted`'s docstring cites as the ceiling ELBO(adapted) <= log p(y), computed on the device.

A step is two launches: the existing resampling launch K2 on the log-weights (its row log-sum-exp is the step's evidence
increment) and K31 (`aesmc_switching_kalman_step`): the gather through the ancestors, the inverse-CDF regime draw, the
Kalman predict, the Dy x Dy Cholesky factor, two triangular solves and the rank-Dy downdate, one lane per particle in
float64.  The NumPy contract of both is `aesmc_amd.testing.rao_blackwell`.

    SwitchingLinearGaussian    the model
    switching_filter           the bootstrap on the regimes described above
    adapted_switching_filter   the look-ahead form: with M <= 16 regimes one Kalman prediction per regime gives every particle
                               p(y_t | s_t = j, history) for all j, hence the exact first-stage weight p(y_t | history) and the
                               exact regime posterior.  A step is the look-ahead K32 (`aesmc_switching_lookahead`) on the stored
                               system, K2 on its log-weights, and K33 (`aesmc_switching_kalman_draw`: K31 with the regime drawn
                               from the ancestor's posterior row).  The weights after the draw are all equal; at T = 1 the
                               evidence is exact for any K, and a regime change is met in the step where it happens (Chen &
                               Liu 2000; Doucet, Gordon & Krishnamurthy 2001; Pitt & Shephard 1999)
    discrete_switching_filter  the discrete particle filter (Fearnhead & Clifford 2003): no regime is drawn.  Every particle
                               proposes all M successor regimes with their exact weights (K43,
                               `aesmc_switching_lookahead_scores`: K32's scores themselves) and K of the K M candidates survive
                               under optimal resampling (K44, `aesmc_switching_optimal_resample`: heavier than a threshold c as
                               they are, the rest thinned by one stratified draw to the weight c), then K31 forced to the
                               survivors' regimes.  No regime history appears twice, the evidence stays unbiased and is
                               exact while M^T <= K
    kalman_log_likelihood      one regime: the exact log p(y)
    unpack_covariance          packed lower triangles -> symmetric matrices
    switching_backward_simulate   Rao-Blackwellised backward simulation (Fong, Godsill, Doucet & West 2002; Whiteley, Andrieu
                               & Doucet 2010; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016) over the stored systems of
                               either filter: equally weighted regime trajectories from p(s_{0:T-1} | y_{0:T-1}) and the
                               smoothed regime probabilities p(s_t | y_{0:T-1}) — offline segmentation.  With z integrated
                               out the regimes are not Markov, so `smoothing.backward_simulate` has no transition to score:
                               every trajectory carries backwards a quadratic summary (Om, lam, c) of its future
                               observations (K34, `aesmc_switching_information_step`, one lane per trajectory) and every
                               stored particle is scored by a closed-form Gaussian integral against it (K35,
                               `aesmc_switching_backward_scores`, one lane per particle walking a tile of trajectories);
                               K21 then draws one particle per trajectory
    switching_smooth           a filter, then that
    conditional_kalman_filter  the exact Kalman filter of z along GIVEN regime paths, one per trajectory: K31 with the regime
                               forced; log p(y | s_{0:T-1}) per trajectory
    switching_state_smooth     the smoothed continuous state from regime trajectories: E[z_t | y], Cov[z_t | y] and the lag-one
                               moments E[z_{t+1} z_t^T | y] (what an EM M-step for A, b, q needs) as the average of the EXACT
                               state smoothers along the trajectories — still only the regimes are sampled.  Per timestep
                               K34 along the trajectory's regimes and K36 (`aesmc_switching_smooth_combine`, one lane per
                               trajectory): the two-filter combination of the filter's N(m, P) with K34's information, which
                               factors I + F^T P F (pivots at least 1) and never a predicted covariance — q = 0 components
                               and P = 0 are fine where an RTS step would divide by a singular matrix
    switching_smooth_states    a filter, the backward simulation, then that (examples/slds_em.py: Monte Carlo EM on it)
    switching_sample_states    a DRAW of the continuous state along given regime paths, z_{0:T-1} ~ p(z | s_{0:T-1}, y): forward
                               filtering, backward sampling (Fruehwirth-Schnatter 1994; Carter & Kohn 1994).
                               `conditional_kalman_filter` forward, then the whole backward pass in ONE launch (K47,
                               `aesmc_switching_state_draw`: one lane per trajectory walks t = T-1 .. 0 with z_{t+1} in
                               registers — a measurement update of N(m_t, P_t) by z_{t+1}, then an affine draw; both
                               factorisations drop pivots as K34's, so q = 0 components and P = 0 are fine).  With
                               `switching_particle_gibbs` and conjugate parameter draws: Gibbs over regimes, states and all
                               ten parameters (examples/slds_gibbs_full.py)
    conditional_switching_filter   one sweep of particle Gibbs with ancestor sampling on the regimes (Andrieu, Doucet &
                               Holenstein 2010; Whiteley, Andrieu & Doucet 2010; Lindsten et al. 2016): a conditional
                               Rao-Blackwellised filter whose last slot carries a reference regime path — a Markov kernel on
                               paths that leaves p(s_{0:T-1} | y) invariant for ANY number of particles, O(K) per step where the
                               smoother above costs O(N K).  Backwards K34 along the reference; per step K37
                               (`aesmc_switching_conditional_ancestor_index`: K26 with the pinned slot scored by K35's integral)
                               and K38 (`aesmc_switching_kalman_conditional_step`: K31 with that slot's regime pinned).
                               With lookahead=True the conditional form of `adapted_switching_filter`: the free slots
                               resample on p(y_t | history) and draw the regime from its exact posterior, the systems stay
                               equally weighted, the pinned slot's ancestor score carries no weight.  Per step K48
                               (`aesmc_switching_lookahead_conditional_ancestor_index`: K32 and K37 in one launch) and K49
                               (`aesmc_switching_kalman_conditional_draw`: K33 with slot K-1 pinned)
    collapsed_switching_filter   the DETERMINISTIC collapsed-mixture filter everyone else uses on this model class: GPB2,
                               which is Kim's filter (Kim 1994; Kim & Nelson 1999), and its first-order cousin IMM (Blom &
                               Bar-Shalom 1988).  M Gaussians per series, no particles, no random numbers, M^2 (IMM: M)
                               Kalman updates per step: K31 with the regime forced on the pair slots, then K50
                               (`aesmc_switching_collapse`: the moment-matching collapse of every regime's mixture into one
                               Gaussian).  A noise-free approximate evidence and segmentation — exact for T <= 2 (IMM: T = 1),
                               for one regime and for dynamics shared across regimes — to hold the particle filters against
    collapsed_switching_smooth   Kim's smoother on top of it: backwards, K51 (`aesmc_switching_pair_smooth`: a
                               Rauch-Tung-Striebel step between component i at t and regime j's smoothed component at t+1,
                               K47's pivot rule) and K50 over j.  Smoothed regime, pair and state moments without a random
                               number: a good start for particle Gibbs for free
    switching_particle_gibbs   the chain of such sweeps; its paths are what `switching_state_smooth` takes
                               (examples/slds_gibbs.py: Gibbs over Pi with Dirichlet rows)
    switching_forecast         the predictive distributions of the steps after the last observation, from either filter's
                               last stored system: steps with nothing observed
    switching_expected_statistics   EM's E-step reduction: the expected complete-data sufficient statistics per regime, summed
                               over time, batch rows and trajectories, from the per-trajectory smoothed moments.  One launch
                               per timestep (K45 `aesmc_switching_moment_statistics`, under a mask K46
                               `aesmc_switching_masked_moment_statistics`): one lane per trajectory forms its terms, the
                               float64 matrix cores sum them against the indicator of the regime — no atomics, one fixed
                               order, the same inputs give the same bits
    switching_m_step           the closed-form M-step for every parameter (pi0, Pi, m0, s0, A, b, q, C, d, r) on those sums:
                               a new model (examples/slds_em_full.py)
    switching_score            the score by Fisher's identity on the same sums, for a gradient optimiser: no adjoint of the
                               filters' Cholesky chains is needed

Missing observations: every function above takes `observed=`, per timestep None or a torch.bool [batch_size, Dy] mask.  For a
batch row a step is then the step of the model with that row's unmeasured components deleted from C, d, r and y — exact, as
a Kalman filter treats a gap: no innovation from an unmeasured component, the prediction where nothing was measured.  The
three kernels that read y have a masked form each (K39 `aesmc_switching_kalman_masked_step`, K40
`aesmc_switching_masked_lookahead`, K41 `aesmc_switching_masked_information_step`: the same bodies with the deleted rows of
the innovation selected to those of the identity), and so has K36, which reads no y but adds the information C^T R^-1 C of
y_{t+1} to its cross-covariance (K42 `aesmc_switching_masked_smooth_combine`: only the measured components add theirs).
The value of y at an unmeasured position is never used and may be NaN.
A NaN at a MEASURED position is still an error.  The contract is `aesmc_amd.testing.switching_missing`.

The reference has no counterpart; this module adds to its interface and changes none of it.
"""
import math

import torch

from . import _kernels
from . import _lib
from . import _ops
from . import _syncfree
from . import inference
from . import statistics

MAX_LATENT_DIM, MAX_OBSERVATION_DIM, MAX_REGIMES = 8, 8, 16      # aesmc_switching_max_*() of the library
_COVERED = ("covered: switching linear-Gaussian models with at most {} regimes, a latent of at most {} values and an "
            "observation of at most {} values, constant in time; observations [batch_size, Dy] of float32 or float64 on "
            "the HIP device, with an optional torch.bool mask of the same shape per timestep (observed=) for components "
            "that were not measured".format(MAX_REGIMES, MAX_LATENT_DIM, MAX_OBSERVATION_DIM))


def _refuse(what):
    raise NotImplementedError("aesmc_amd.rao_blackwell: {} is not implemented; {}".format(what, _COVERED))


class SwitchingLinearGaussian(torch.nn.Module):
    """A switching linear-Gaussian state-space model with M regimes, latent z in R^D and observation y in R^Dy.

    pi0 [M], Pi [M,M] (rows: from-regime); m0 [D], s0 (one value or D); A [M,D,D], b [M,D], q [M,D]; C [M,Dy,D], d [M,Dy],
    r [M,Dy].  A leading extent of 1 in place of M means shared across regimes.  Every component of y_t is part of the model;
    which of them were measured at a step is the filters' `observed=`, not the model's.  Everything is held as a float64 buffer
    (`.to(device)` moves the model).  The filters are not differentiable — with one exception,
    `collapsed_switching_log_likelihood`, which takes the ten tensors themselves and returns the collapsed-mixture evidence
    with its graph (examples/slds_sgd.py) — and the buffers are no parameters: a model is otherwise learned by EM —
    `switching_smooth_states` gives the E-step's smoothed moments E[z_t z_t^T | y], E[z_{t+1} z_t^T | y] and regime
    trajectories, `switching_expected_statistics` reduces them to the expected sufficient statistics per regime and
    `switching_m_step` builds a new model from those in closed form (examples/slds_em_full.py; examples/slds_em.py does the
    M-step for Pi, A and b by hand) — or by a gradient optimiser on `switching_score`, the score by Fisher's identity — or
    sampled: `switching_particle_gibbs` draws the regimes, `switching_sample_states` the states along them, and the
    parameters given both are conjugate (examples/slds_gibbs_full.py)."""

    def __init__(self, pi0, Pi, m0, s0, A, b, q, C, d, r):
        super().__init__()
        for name, value in (("pi0", pi0), ("Pi", Pi), ("m0", m0), ("s0", s0), ("A", A), ("b", b), ("q", q), ("C", C),
                            ("d", d), ("r", r)):
            self.register_buffer(name, torch.as_tensor(value).detach().to(torch.float64).clone())

    @property
    def num_regimes(self):
        return self.pi0.numel()

    @property
    def latent_dim(self):
        return self.A.size(-1) if self.A.dim() == 3 else 0

    @property
    def observation_dim(self):
        return self.C.size(-2) if self.C.dim() == 3 else 0

    def operands(self):
        """The model as a step takes it: a dict of dense float64 tensors on the buffers' device — pi0 [M], Pi [M,M], their
        cumulative rows cdf0 [M] and cdf [M,M] (torch.cumsum on the host, the last entry set to 1), m0 [D], s0 [D], and A,
        b, q, C, d, r expanded to M regimes.  Validates: ValueError for shapes that disagree, for probabilities that are
        negative or do not sum to 1 within 1e-12 and for scales that are not finite; NotImplementedError naming the
        covered class for anything past the limits.  One copy to the host (the probabilities and the scales together); the
        cumulative rows are copied back."""
        M, D, Dy = self.num_regimes, self.latent_dim, self.observation_dim
        if self.pi0.dim() != 1 or M < 1 or tuple(self.Pi.shape) != (M, M):
            raise ValueError("SwitchingLinearGaussian: pi0 must be [M] and Pi [M, M], got {} and {}".format(
                tuple(self.pi0.shape), tuple(self.Pi.shape)))
        if self.A.dim() != 3 or self.C.dim() != 3 or D < 1 or Dy < 1 or self.A.size(1) != D or self.C.size(2) != D:
            raise ValueError("SwitchingLinearGaussian: A must be [M, D, D] and C [M, Dy, D], got {} and {}".format(
                tuple(self.A.shape), tuple(self.C.shape)))
        if M > MAX_REGIMES:
            _refuse("a model of {} regimes (M > {})".format(M, MAX_REGIMES))
        if D > MAX_LATENT_DIM:
            _refuse("a latent of {} values (D > {})".format(D, MAX_LATENT_DIM))
        if Dy > MAX_OBSERVATION_DIM:
            _refuse("an observation of {} values (Dy > {})".format(Dy, MAX_OBSERVATION_DIM))
        shapes = {"A": (M, D, D), "b": (M, D), "q": (M, D), "C": (M, Dy, D), "d": (M, Dy), "r": (M, Dy)}
        out = {}
        for name, shape in shapes.items():
            value = getattr(self, name)
            if value.dim() != len(shape) or value.size(0) not in (1, M) or tuple(value.shape[1:]) != shape[1:]:
                raise ValueError("SwitchingLinearGaussian: {} must be {} (or a leading 1: shared across regimes), got {}"
                                 .format(name, shape, tuple(value.shape)))
            out[name] = value.expand(shape).contiguous()
        if tuple(self.m0.shape) != (D,):
            raise ValueError("SwitchingLinearGaussian: m0 must be [{}], got {}".format(D, tuple(self.m0.shape)))
        if self.s0.numel() not in (1, D):
            raise ValueError("SwitchingLinearGaussian: s0 must hold one value or {}, got {}".format(D, self.s0.numel()))
        out["m0"] = self.m0.contiguous()
        out["s0"] = self.s0.reshape(-1).expand(D).contiguous()
        device = self.pi0.device
        # ONE copy to the host: the probabilities (validated and accumulated there) with the scales behind them
        host = torch.cat([self.pi0.reshape(-1), self.Pi.reshape(-1)] +
                         [out[name].reshape(-1) for name in ("s0", "q", "r")]).cpu()
        pi0, Pi, scales = host[:M].clone(), host[M:M + M * M].reshape(M, M).clone(), host[M + M * M:]
        for name, p in (("pi0", pi0), ("Pi", Pi)):
            if not bool(torch.isfinite(p).all()) or bool((p < 0).any()):
                raise ValueError("SwitchingLinearGaussian: {} holds a negative or non-finite probability".format(name))
            if bool(((p.sum(dim=-1) - 1.0).abs() > 1e-12).any()):
                raise ValueError("SwitchingLinearGaussian: {} must sum to 1 within 1e-12 along its last dimension".format(
                    name))
        if not bool(torch.isfinite(scales).all()):
            raise ValueError("SwitchingLinearGaussian: a scale is not finite")
        cdf0, cdf = torch.cumsum(pi0, dim=-1), torch.cumsum(Pi, dim=-1)
        cdf0[-1] = 1.0
        cdf[:, -1] = 1.0
        out.update(pi0=self.pi0.contiguous(), Pi=self.Pi.contiguous(), cdf0=cdf0.to(device), cdf=cdf.to(device))
        return out

    def simulate(self, num_timesteps, batch_size, seed=None, return_latents=False):
        """Draws `batch_size` series of `num_timesteps` observations from the model (torch's CPU generator; `seed` fixes
        it): a list of [batch_size, Dy] float64 tensors on the model's device — with `return_latents`, (observations,
        regimes: T x int64 [batch_size], states: T x [batch_size, D]) instead."""
        ops = {name: value.cpu() for name, value in self.operands().items()}
        generator = torch.Generator()
        if seed is not None:
            generator.manual_seed(int(seed))
        D, Dy = self.latent_dim, self.observation_dim
        device = self.pi0.device
        normal = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=generator)
        observations, regimes, states = [], [], []
        for time in range(num_timesteps):
            if time == 0:
                s = torch.multinomial(ops["pi0"].expand(batch_size, -1), 1, generator=generator).squeeze(1)
                z = ops["m0"] + ops["s0"] * normal(batch_size, D)
            else:
                s = torch.multinomial(ops["Pi"][s], 1, generator=generator).squeeze(1)
                z = torch.einsum("bij,bj->bi", ops["A"][s], z) + ops["b"][s] + ops["q"][s] * normal(batch_size, D)
            y = torch.einsum("bij,bj->bi", ops["C"][s], z) + ops["d"][s] + ops["r"][s] * normal(batch_size, Dy)
            observations.append(y.to(device)), regimes.append(s.to(device)), states.append(z.to(device))
        return (observations, regimes, states) if return_latents else observations


def unpack_covariance(packed, dim):
    """[..., D(D+1)/2] packed lower triangles (element (i,j), i >= j, at i(i+1)/2 + j) -> [..., D, D] symmetric."""
    rows, cols = torch.tril_indices(dim, dim, device=packed.device)
    full = packed.new_zeros(packed.shape[:-1] + (dim, dim))
    full[..., rows, cols] = packed
    full[..., cols, rows] = packed
    return full


def _moments(regimes, means, covariances, log_weights, num_regimes):
    """(filtered_mean [T,B,D], filtered_covariance [T,B,D,D], regime_probabilities [T,B,M]) of the stored systems: the
    weighted summaries are `statistics.empirical_mean`'s (kernel K7 on the device), the rest plain torch."""
    filtered_mean, filtered_cov, probabilities = [], [], []
    for regime, mean, cov, log_w in zip(regimes, means, covariances, log_weights):
        D = mean.size(-1)
        average = statistics.empirical_mean(mean, log_w)
        second = unpack_covariance(cov, D) + mean.unsqueeze(-1) * mean.unsqueeze(-2)
        second = statistics.empirical_mean(second.reshape(second.shape[:2] + (D * D,)), log_w).reshape(-1, D, D)
        one_hot = torch.nn.functional.one_hot(regime.to(torch.int64), num_regimes).to(torch.float64)
        filtered_mean.append(average)
        filtered_cov.append(second - average.unsqueeze(-1) * average.unsqueeze(-2))
        probabilities.append(statistics.empirical_mean(one_hot, log_w))
    return torch.stack(filtered_mean), torch.stack(filtered_cov), torch.stack(probabilities)


def _check_arguments(name, observations, num_particles, regime_uniforms, resampling):
    """(T, K, stratified) of a filter's arguments: what is checked before the provider is asked for anything."""
    from . import distributed
    num_timesteps, num_particles = len(observations), int(num_particles)
    if num_timesteps == 0:
        raise ValueError("{}: observations must hold at least one timestep".format(name))
    if num_particles < 1:
        raise ValueError("{}: num_particles must be at least 1".format(name))
    if regime_uniforms is not None and len(regime_uniforms) != num_timesteps:
        raise ValueError("{}: regime_uniforms must hold one tensor per timestep ({}), got {}".format(
            name, num_timesteps, len(regime_uniforms)))
    stratified = inference._resolve_resampling(resampling) == "stratified"
    if regime_uniforms is None and distributed.active_shard() is not None:
        raise NotImplementedError(
            "aesmc_amd.rao_blackwell: drawing the regime uniforms inside distributed.shard_scope is not implemented: a "
            "sharded run reproduces the unsharded one through the global block of host uniforms every rank draws, which "
            "per-particle device draws do not have. Pass regime_uniforms when sharding.")
    return num_timesteps, num_particles, stratified


def _check_observations(name, provider, observations, model, num_particles):
    """(batch_size, device) of the observations, or the refusal: [batch_size, Dy] tensors the provider's step covers."""
    M, D, Dy = model.num_regimes, model.latent_dim, model.observation_dim
    for y in observations:
        if not torch.is_tensor(y) or y.dim() != 2 or y.size(1) != Dy or y.size(0) != observations[0].size(0):
            raise ValueError("{}: observations must be [batch_size, {}] tensors".format(name, Dy))
    batch_size, device = observations[0].size(0), observations[0].device
    if provider.name == "hip":
        _kernels._require_hip(observations[0], "observations")      # (no CPU fallback)
    if not provider.switching_covers(observations[0], M, D, Dy, num_particles):
        _refuse("these observations ({} {} on {})".format(tuple(observations[0].shape), observations[0].dtype, device))
    return batch_size, device


def _observed_steps(name, observed, observations):
    """time -> the keywords of that step's provider calls: {} where the step is fully observed (today's entries and
    results, bit for bit), {"observed": mask} where a mask is given (the masked entries K39, K40, K41).  observed: None, or
    a length-T sequence whose entries are None or torch.bool tensors of the observation's shape on its device; ValueError
    otherwise.  Called once the observations are validated; reads nothing from the device."""
    if observed is None:
        return lambda time: {}
    try:
        length = len(observed)
    except TypeError:
        length = -1
    if length != len(observations):
        raise ValueError("{}: observed must be None or hold one entry per timestep ({}), got {}".format(
            name, len(observations), "{} entries".format(length) if length >= 0 else type(observed).__name__))
    shape, device = tuple(observations[0].shape), observations[0].device
    for time in range(length):
        mask = observed[time]
        if mask is not None and not (torch.is_tensor(mask) and mask.dtype == torch.bool and tuple(mask.shape) == shape and
                                     mask.device == device):
            raise ValueError("{}: observed[{}] must be None or {} torch.bool on {}, got {}".format(
                name, time, shape, device, "{} {} on {}".format(tuple(mask.shape), mask.dtype, mask.device)
                if torch.is_tensor(mask) else type(mask).__name__))
    return lambda time: {} if observed[time] is None else {"observed": observed[time]}


def _regime_draws(name, regime_uniforms, shape, device):
    """time -> the step's regime uniforms: fresh from torch's device generator, or the replayed tensor, validated."""
    def draw(time):
        if regime_uniforms is None:
            return torch.rand(shape, dtype=torch.float64, device=device)
        u = regime_uniforms[time]
        if not torch.is_tensor(u) or tuple(u.shape) != shape or u.dtype != torch.float64 or u.device != device:
            raise ValueError("{}: regime_uniforms[{}] must be {} float64 on {}".format(name, time, shape, device))
        return u
    return draw


def _resampling_uniforms(feed, stratified, batch_size, num_particles, num_timesteps, device):
    """(feed, the next step's resampling uniforms): the feed is `infer`'s (an override, or the scheme's own, made at the
    first resampling step), and what it returns must have the scheme's shape."""
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
    return feed, uniforms


def switching_filter(observations, model, num_particles, resampling=None, regime_uniforms=None, return_moments=False,
                     return_latents=False, observed=None):
    """Runs the Rao-Blackwellised particle filter of a `SwitchingLinearGaussian`.

    observations: length-T sequence of [batch_size, Dy] tensors (float32 or float64) on the model's device.
    num_particles: K.
    resampling: 'systematic', 'stratified' or None (`settings.current().resampling`), as `infer` — the uniforms come from
        the same feeds (`inference.uniform_feed(...)` overrides them), and 'stratified' inside `distributed.shard_scope`
        raises.  Every step resamples.
    regime_uniforms: None — torch.rand((batch_size, num_particles), float64) per step on the device (seed with
        torch.manual_seed); or a length-T sequence of such tensors (replay).  None inside `distributed.shard_scope` raises
        NotImplementedError for the reason stratified resampling does: a per-particle device draw has no global block
        that every rank could cut its rows from.
    return_moments: also filtered_mean [T,batch_size,D], filtered_covariance [T,batch_size,D,D] (the mixture's: sum_k w_k
        (P_k + m_k m_k^T) - mean mean^T) and regime_probabilities [T,batch_size,M].
    return_latents: also `latents`: the regime genealogy (`inference.get_resampled_latents` of the stored regimes).
    observed: None — every component of every y_t was measured; or a length-T sequence whose entries are None (that step
        fully observed) or torch.bool [batch_size, Dy] tensors on the device, True where the component was measured.  For
        batch row b a step is then the step of the model with that row's unmeasured components deleted from C, d, r and
        y (the masked kernels K39 - K41): a component that was not measured contributes no innovation, a step with
        nothing measured is the prediction (log-weight 0).  The value of y at an unmeasured position is never used and may
        be NaN or Inf.  None, or only None entries, is today's path bit for bit.

    Returns a dict: log_marginal_likelihood [batch_size] float64 (unbiased for p(y_0..y_{T-1}); exact for M = 1); regimes (T
    int32 [batch_size, K]), means (T float64 [batch_size, K, D]), covariances (T float64 [batch_size, K, D(D+1)/2]: packed
    lower triangles, `unpack_covariance`), log_weights (T float64 [batch_size, K]) — the stored, un-resampled particle
    systems; ancestral_indices (T-1 int64 [batch_size, K], `infer`'s convention); log_weight (the last of log_weights).

    ValueError for an invalid model (`SwitchingLinearGaussian.operands`), T == 0, K < 1 and feeds of the wrong shape;
    NotImplementedError naming the covered class for anything past the limits.  An innovation covariance that is not
    positive definite gives NaN log-weights and FloatingPointError, a row without a finite maximum RuntimeError — read
    once, at the end; an exception on the way discards whatever was flagged.  No host synchronisation inside the step
    loop.  Runs under torch.no_grad(): NOT differentiable."""
    num_timesteps, num_particles, stratified = _check_arguments("switching_filter", observations, num_particles,
                                                                regime_uniforms, resampling)
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops = model.operands()      # validation, expansion and the cumulative rows: once, before the loop
            M = model.num_regimes
            batch_size, device = _check_observations("switching_filter", provider, observations, model, num_particles)
            mask = _observed_steps("switching_filter", observed, observations)
            draw = _regime_draws("switching_filter", regime_uniforms, (batch_size, num_particles), device)
            log_z = torch.zeros(batch_size, dtype=torch.float64, device=device)
            regimes, means, covariances, log_weights, ancestral = [], [], [], [], []
            state, index, feed = None, None, None
            for time in range(num_timesteps):
                if time > 0:
                    feed, uniforms = _resampling_uniforms(feed, stratified, batch_size, num_particles, num_timesteps, device)
                    index, lse, _ = _ops.resample_step(log_weights[-1], uniforms, None, want_lse=True)
                    index = _kernels.as_index(index)
                    log_z = log_z + (lse.to(torch.float64) - math.log(num_particles))
                    ancestral.append(index)
                regime, mean, cov, log_w = provider.switching_kalman_step(ops, state, index, draw(time),
                                                                          observations[time], **mask(time))
                state = (regime, mean, cov)
                regimes.append(regime), means.append(mean), covariances.append(cov), log_weights.append(log_w)
            log_z = log_z + (_ops.row_logsumexp(log_weights[-1]).to(torch.float64) - math.log(num_particles))
            out = {"log_marginal_likelihood": log_z, "regimes": regimes, "means": means, "covariances": covariances,
                   "log_weights": log_weights, "ancestral_indices": ancestral, "log_weight": log_weights[-1]}
            if return_moments:
                out["filtered_mean"], out["filtered_covariance"], out["regime_probabilities"] = _moments(
                    regimes, means, covariances, log_weights, M)
            if return_latents:
                out["latents"] = inference.get_resampled_latents(regimes, ancestral)
            inference._raise_for_flags(provider.read_flags(device))
            # (the last step's log-weights meet no resampling launch: a NaN among them is reported here, after the one read)
            if bool(torch.isnan(log_z).any()):
                raise FloatingPointError("log_weight contains nan element(s)")
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


def adapted_switching_filter(observations, model, num_particles, resampling=None, regime_uniforms=None,
                             return_moments=False, return_latents=False, observed=None):
    """Runs the fully adapted (look-ahead) Rao-Blackwellised filter of a `SwitchingLinearGaussian`: every step resamples on
    the exact first-stage weights p(y_t | history) and draws the regime from its exact posterior p(s_t | history, y_t).

    Arguments, validation, refusals and feeds as `switching_filter` (T - 1 blocks of resampling uniforms, T of regime
    uniforms); `observed` as there too (K40 and K39 in place of K32 and K33): at a step where a row measured nothing its
    first-stage weights are all equal and the regime is drawn from the transition's row.

    Returns a dict: log_marginal_likelihood [batch_size] float64 (unbiased for p(y_0..y_{T-1}); exact for M = 1 and, for any
    K, at T = 1); regimes (T int32 [batch_size, K]), means, covariances (packed, as `switching_filter`'s) — the T stored,
    EQUALLY WEIGHTED systems after the draw; first_stage_log_weights (T float64 [batch_size, K]: the look-ahead of step t on
    system t-1, of step 0 on the prior, where all K are equal); ancestral_indices (T-1 int64 [batch_size, K]).  With
    return_moments, `switching_filter`'s three moments under equal weights; with return_latents, the regime genealogy.

    An innovation covariance that is not positive definite under a regime of positive prior probability gives a NaN
    first-stage weight and FloatingPointError (under a regime of probability zero it is ignored); flags are read once, at the
    end; an exception on the way discards whatever was flagged.  No host synchronisation inside the step loop.  Runs under
    torch.no_grad(): NOT differentiable."""
    num_timesteps, num_particles, stratified = _check_arguments("adapted_switching_filter", observations, num_particles,
                                                                regime_uniforms, resampling)
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops = model.operands()
            M = model.num_regimes
            batch_size, device = _check_observations("adapted_switching_filter", provider, observations, model,
                                                     num_particles)
            mask = _observed_steps("adapted_switching_filter", observed, observations)
            draw = _regime_draws("adapted_switching_filter", regime_uniforms, (batch_size, num_particles), device)
            log_pi0, log_Pi = torch.log(ops["pi0"]), torch.log(ops["Pi"])      # (-inf where a probability is 0) once
            log_z = torch.zeros(batch_size, dtype=torch.float64, device=device)
            regimes, means, covariances, first_stage, ancestral = [], [], [], [], []
            state, feed = None, None
            for time in range(num_timesteps):
                regime_u = draw(time)      # (a replayed tensor of the wrong shape is refused before the step's launches)
                log_w, cdf = provider.switching_lookahead(ops, log_pi0 if time == 0 else log_Pi, state, observations[time],
                                                          num_particles=num_particles, **mask(time))
                if time == 0:
                    index, lse = None, _ops.row_logsumexp(log_w)
                else:
                    feed, uniforms = _resampling_uniforms(feed, stratified, batch_size, num_particles, num_timesteps, device)
                    index, lse, _ = _ops.resample_step(log_w, uniforms, None, want_lse=True)
                    index = _kernels.as_index(index)
                    ancestral.append(index)
                log_z = log_z + (lse.to(torch.float64) - math.log(num_particles))
                regime, mean, cov, _ = provider.switching_kalman_draw(ops, state, index, regime_u, cdf, observations[time],
                                                                      **mask(time))
                state = (regime, mean, cov)
                regimes.append(regime), means.append(mean), covariances.append(cov), first_stage.append(log_w)
            out = {"log_marginal_likelihood": log_z, "regimes": regimes, "means": means, "covariances": covariances,
                   "first_stage_log_weights": first_stage, "ancestral_indices": ancestral}
            if return_moments:
                equal = torch.zeros((batch_size, num_particles), dtype=torch.float64, device=device)
                out["filtered_mean"], out["filtered_covariance"], out["regime_probabilities"] = _moments(
                    regimes, means, covariances, [equal] * num_timesteps, M)
            if return_latents:
                out["latents"] = inference.get_resampled_latents(regimes, ancestral)
            inference._raise_for_flags(provider.read_flags(device))
            # (step 0's first-stage weights meet no resampling launch: a NaN among them is reported here, after the one read)
            if bool(torch.isnan(log_z).any()):
                raise FloatingPointError("log_weight contains nan element(s)")
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


def discrete_switching_filter(observations, model, num_particles, uniforms=None, return_moments=False,
                              return_latents=False, observed=None):
    """Runs the discrete particle filter (Fearnhead & Clifford 2003) of a `SwitchingLinearGaussian`: no regime is drawn.
    Every particle proposes ALL M successor regimes with their exact weights (K43, `aesmc_switching_lookahead_scores`: K32's
    scores, which that kernel computes and discards), and K of the K M candidates survive under optimal resampling (K44,
    `aesmc_switching_optimal_resample`): every candidate heavier than a threshold c as it is, the rest thinned by one
    stratified draw to the weight c each.  K31, with the regime forced and `idx = parent`, then gives the survivors their
    Kalman moments.  With z integrated out two particles of one regime history are one particle; here no history appears
    twice, the resampling is unbiased — so is the evidence — and while M^(t+1) <= K nothing is discarded: the filter is exact.

    observations, model, num_particles, return_moments, return_latents, observed: as `switching_filter`'s (with `observed` the
        masked kernels: K40's body for the scores and K39 for the step).
    uniforms: None — torch.rand(batch_size, float64) per step on the device (seed with torch.manual_seed), ONE uniform per
        batch row and step; or a length-T sequence of such tensors (replay).  None inside `distributed.shard_scope` raises
        NotImplementedError, as `regime_uniforms` does there.

    Returns a dict in `switching_filter`'s format — what `switching_backward_simulate` and `switching_forecast` take
    unchanged (`switching_state_smooth` takes the trajectories drawn from it): log_marginal_likelihood [batch_size] float64 (the sum of K44's evidence increments;
    unbiased, and exact while M^T <= K); regimes, means, covariances (T stored systems); log_weights (T float64
    [batch_size, K], NORMALISED: their log-sum-exp is 0; -inf in a dead slot — with fewer than K live candidates the
    remaining slots carry a copy of slot 0's state and weight zero); ancestral_indices (T-1 int64 [batch_size, K]: K44's
    parents of steps 1 .. T-1); log_weight (the last of log_weights); num_live (T int32 [batch_size]: the slots that carry
    weight).  With return_moments and return_latents, `switching_filter`'s additions.

    ValueError for an invalid model, T == 0, K < 1 and uniforms of the wrong length or shape; NotImplementedError naming the
    covered class for anything past the limits, and for K M above the candidates K44 keeps in LDS (16384).  A NaN score (an
    innovation covariance that is not positive definite under a regime of positive prior probability) raises
    FloatingPointError, a step without a candidate of positive weight RuntimeError — the flags are read once, at the end; an
    exception on the way discards whatever was flagged.  No host synchronisation inside the step loop.  Runs under
    torch.no_grad(): NOT differentiable."""
    name = "discrete_switching_filter"
    if uniforms is not None and len(uniforms) != len(observations):
        raise ValueError("{}: uniforms must hold one tensor per timestep ({}), got {}".format(name, len(observations),
                                                                                              len(uniforms)))
    num_timesteps, num_particles, _ = _check_arguments(name, observations, num_particles, uniforms, None)
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops = model.operands()
            M = model.num_regimes
            batch_size, device = _check_observations(name, provider, observations, model, num_particles)
            if not provider.switching_optimal_resample_covers(num_particles, M, num_particles, batch_size):
                _refuse("{} particles of {} regimes ({} candidates per batch row; optimal resampling keeps at most {} in "
                        "LDS)".format(num_particles, M, num_particles * M, provider.switching_optimal_resample_max_candidates()))
            mask = _observed_steps(name, observed, observations)
            draw = _regime_draws(name, uniforms, (batch_size,), device)
            log_pi0, log_Pi = torch.log(ops["pi0"]), torch.log(ops["Pi"])      # (-inf where a probability is 0) once
            edges = (torch.arange(M, dtype=torch.float64, device=device) + 1.0) / M
            forced = dict(ops, cdf0=edges, cdf=edges.expand(M, M).contiguous())      # `_conditional_filter`'s forced draw
            log_z = torch.zeros(batch_size, dtype=torch.float64, device=device)
            regimes, means, covariances, log_weights, ancestral, num_live = [], [], [], [], [], []
            state, log_w = None, None
            for time in range(num_timesteps):
                u = draw(time)      # (a replayed tensor of the wrong shape is refused before the step's launches)
                scores, _ = provider.switching_lookahead_scores(ops, log_pi0 if time == 0 else log_Pi, state,
                                                                observations[time], num_particles=1 if time == 0 else None,
                                                                **mask(time))
                parent, chosen, log_w, lse, count = provider.switching_optimal_resample(log_w, scores, u, num_particles)
                log_z = log_z + lse
                if time > 0:
                    ancestral.append(parent)
                regime, mean, cov, _ = provider.switching_kalman_step(
                    forced, state, parent if time > 0 else None, (chosen.to(torch.float64) + 0.5) / M, observations[time],
                    **mask(time))
                state = (regime, mean, cov)
                regimes.append(regime), means.append(mean), covariances.append(cov), log_weights.append(log_w)
                num_live.append(count)
            out = {"log_marginal_likelihood": log_z, "regimes": regimes, "means": means, "covariances": covariances,
                   "log_weights": log_weights, "ancestral_indices": ancestral, "log_weight": log_weights[-1],
                   "num_live": num_live}
            if return_moments:
                out["filtered_mean"], out["filtered_covariance"], out["regime_probabilities"] = _moments(
                    regimes, means, covariances, log_weights, M)
            if return_latents:
                out["latents"] = inference.get_resampled_latents(regimes, ancestral)
            inference._raise_for_flags(provider.read_flags(device))
            if bool(torch.isnan(log_z).any()):
                raise FloatingPointError("log_weight contains nan element(s)")
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


def _stored_systems(name, filtered, num_timesteps, batch_size, latent_dim, device):
    """(regimes, means, covariances, log_weights or None, K) of a filter's dict, validated: T stored systems each."""
    for key in ("regimes", "means", "covariances"):
        if key not in filtered or len(filtered[key]) != num_timesteps:
            raise ValueError("{}: filtered must hold {} '{}' (the dict of switching_filter or adapted_switching_filter "
                             "on these observations)".format(name, num_timesteps, key))
    log_weights = filtered.get("log_weights")
    if log_weights is not None and len(log_weights) != num_timesteps:
        raise ValueError("{}: filtered must hold {} 'log_weights', got {}".format(name, num_timesteps, len(log_weights)))
    regimes, means, covariances = filtered["regimes"], filtered["means"], filtered["covariances"]
    num_particles = regimes[0].size(1) if torch.is_tensor(regimes[0]) and regimes[0].dim() == 2 else -1
    if num_particles < 1:
        raise ValueError("{}: filtered['regimes'] must be [batch_size, num_particles] tensors of at least one particle"
                         .format(name))
    packed = latent_dim * (latent_dim + 1) // 2
    for time in range(num_timesteps):
        wanted = [(regimes[time], (batch_size, num_particles), torch.int32, "regimes"),
                  (means[time], (batch_size, num_particles, latent_dim), torch.float64, "means"),
                  (covariances[time], (batch_size, num_particles, packed), torch.float64, "covariances")]
        if log_weights is not None:
            wanted.append((log_weights[time], (batch_size, num_particles), torch.float64, "log_weights"))
        for tensor, shape, dtype, key in wanted:
            if not torch.is_tensor(tensor) or tuple(tensor.shape) != shape or tensor.dtype != dtype or tensor.device != device:
                raise ValueError("{}: filtered['{}'][{}] must be {} {} on {}".format(name, key, time, shape, dtype, device))
    return regimes, means, covariances, log_weights, num_particles


def switching_backward_simulate(filtered, model, observations, num_trajectories=None, uniforms=None, return_indices=False,
                                observed=None):
    """Rao-Blackwellised backward simulation over the stored systems of one run of `switching_filter` or
    `adapted_switching_filter`: regime trajectories from the joint smoothing distribution p(s_{0:T-1} | y_{0:T-1}).

    filtered: the dict either filter returned for these observations (regimes, means, covariances; with `log_weights` the
        stored systems are weighted by them — `switching_filter`'s — and without that key equally —
        `adapted_switching_filter`'s).
    model, observations: as the filter's.
    num_trajectories: N per batch row (default: the number of particles).  0 gives empty tensors without a launch.
    uniforms: `smoothing.backward_simulate`'s convention — None: one torch.rand((batch_size, N), float64) block per
        timestep on the device, drawn for t = T-1 first and t = 0 last (seed with torch.manual_seed); or a length-T
        sequence of such blocks, `uniforms[t]` for the draw at time t (replay).  None inside `distributed.shard_scope`
        raises NotImplementedError for that function's reason.
    return_indices: also `indices`: which stored particle each trajectory passes through, T int64 [batch_size, N].
    observed: `switching_filter`'s, and the one the filter ran with (K41 in place of K34).

    At t = T-1 a trajectory draws a stored particle by its weight (K21).  For t = T-2 .. 0 it takes the quadratic summary
    of its future observations one step back under its regime at t+1 (K34), every stored particle of step t is scored
    against it (K35: scores [batch_size, N, K]), and K21 draws one particle per trajectory from those scores (rows
    [batch_size N, K], one trajectory each); the trajectory's regime at t is that particle's.

    Returns a dict: regimes (T int32 [batch_size, N]: trajectory n of row b is (regimes[0][b,n], .., regimes[T-1][b,n]), an
    equally weighted draw) and smoothed_regime_probabilities ([T, batch_size, M] float64: the trajectories' frequencies,
    the estimate of p(s_t = i | y_{0:T-1})); with return_indices, indices.

    ValueError for an invalid model, T == 0, a `filtered` that does not hold T stored systems of the observations' batch
    size, a negative num_trajectories and uniforms of the wrong length or shape; NotImplementedError naming the covered
    class for anything past the limits (also batch_size N K beyond 32-bit element arithmetic).  NaN weights or scores (a
    stored regime outside [0, M) gives them) raise FloatingPointError, a trajectory no stored particle can precede (a row of
    -inf scores: every transition into its regime has probability zero) RuntimeError — read once, at the end; an exception
    on the way discards whatever was flagged.  No host synchronisation inside the loop.  Runs under torch.no_grad(): NOT
    differentiable.  Not sharded, not capturable into a hipGraph."""
    name = "switching_backward_simulate"
    num_timesteps = len(observations)
    if num_timesteps == 0:
        raise ValueError("{}: observations must hold at least one timestep".format(name))
    if uniforms is not None and len(uniforms) != num_timesteps:
        raise ValueError("{}: uniforms must hold one block per timestep ({}), got {}".format(name, num_timesteps,
                                                                                              len(uniforms)))
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops = model.operands()
            M, D, Dy = model.num_regimes, model.latent_dim, model.observation_dim
            # (the observations first, for one particle: what the stored systems must match; their number is checked
            # with the number of trajectories below)
            batch_size, device = _check_observations(name, provider, observations, model, 1)
            mask = _observed_steps(name, observed, observations)
            regimes, means, covariances, log_weights, num_particles = _stored_systems(
                name, filtered, num_timesteps, batch_size, D, device)
            num_trajectories = num_particles if num_trajectories is None else int(num_trajectories)
            if num_trajectories < 0:
                raise ValueError("{}: num_trajectories must not be negative".format(name))
            if uniforms is None:
                from . import distributed
                if distributed.active_shard() is not None:
                    raise NotImplementedError(
                        "aesmc_amd: {} inside distributed.shard_scope draws its uniforms on the device, where no global "
                        "block exists that every rank could cut its rows from. Pass uniforms= (one [batch_size, "
                        "num_trajectories] float64 block per timestep).".format(name))
            if not provider.switching_backward_covers(observations[0], M, D, Dy, num_particles, num_trajectories):
                _refuse("{} trajectories over {} particles in {} batch rows (batch_size * num_trajectories * num_particles "
                        "beyond 32-bit element arithmetic)".format(num_trajectories, num_particles, batch_size))
            shape = (batch_size, num_trajectories)

            def block(time):
                if uniforms is None:
                    return torch.rand(shape, dtype=torch.float64, device=device)
                u = uniforms[time]
                if not torch.is_tensor(u) or tuple(u.shape) != shape or u.dtype != torch.float64 or u.device != device:
                    raise ValueError("{}: uniforms[{}] must be {} float64 on {}".format(name, time, shape, device))
                return u

            if num_trajectories == 0:
                out = {"regimes": [torch.empty(shape, dtype=torch.int32, device=device) for _ in range(num_timesteps)],
                       "smoothed_regime_probabilities": torch.zeros((num_timesteps, batch_size, M), dtype=torch.float64,
                                                                    device=device)}
                if return_indices:
                    out["indices"] = [torch.empty(shape, dtype=torch.int64, device=device) for _ in range(num_timesteps)]
                return out
            log_Pi = torch.log(ops["Pi"])      # (-inf where a probability is 0) once
            equal = None if log_weights is not None else torch.zeros((batch_size, num_particles), dtype=torch.float64,
                                                                     device=device)
            drawn, indices = [None] * num_timesteps, [None] * num_timesteps
            last = num_timesteps - 1
            indices[last], _ = provider.backward_sample(equal if log_weights is None else log_weights[last], None, None,
                                                        None, block(last))
            # (a failed draw is position K, whose payload is particle K-1's by K21's convention; the flag is read at the end)
            drawn[last] = torch.gather(regimes[last], 1, indices[last].clamp(max=num_particles - 1))
            info = None
            for time in range(last - 1, -1, -1):
                u = block(time)      # (a replayed block of the wrong shape is refused before the step's launches)
                omega, lam, c, factor = provider.switching_information_step(ops, drawn[time + 1], info,
                                                                            observations[time + 1], **mask(time + 1))
                info = (omega, lam, c)
                scores = provider.switching_backward_scores(log_Pi, drawn[time + 1], factor, lam,
                                                            (regimes[time], means[time], covariances[time]),
                                                            None if log_weights is None else log_weights[time])
                index, _ = provider.backward_sample(scores.reshape(batch_size * num_trajectories, num_particles), None, None,
                                                    None, u.reshape(batch_size * num_trajectories, 1))
                indices[time] = index.reshape(shape)
                drawn[time] = torch.gather(regimes[time], 1, indices[time].clamp(max=num_particles - 1))
            probabilities = torch.stack([
                torch.nn.functional.one_hot(regime.to(torch.int64).clamp(0, M - 1), M).to(torch.float64).mean(dim=1)
                for regime in drawn])
            out = {"regimes": drawn, "smoothed_regime_probabilities": probabilities}
            if return_indices:
                out["indices"] = indices
            inference._raise_for_flags(provider.read_flags(device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


def switching_smooth(observations, model, num_particles, num_trajectories=None, resampling=None, lookahead=False,
                     observed=None):
    """Runs `switching_filter` (lookahead: `adapted_switching_filter`) and then `switching_backward_simulate` over what it
    stored, both with `observed`.  Returns (that function's dict, the filter's log_marginal_likelihood [batch_size])."""
    run = adapted_switching_filter if lookahead else switching_filter
    filtered = run(observations, model, num_particles, resampling=resampling, observed=observed)
    out = switching_backward_simulate(filtered, model, observations, num_trajectories=num_trajectories, observed=observed)
    return out, filtered["log_marginal_likelihood"]


def _check_regimes(name, regimes, num_timesteps, batch_size, device):
    """N of a regime path per trajectory: T int32 [batch_size, N] tensors on the device."""
    if regimes is None or len(regimes) != num_timesteps:
        raise ValueError("{}: regimes must hold one tensor per timestep ({}), got {}".format(
            name, num_timesteps, 0 if regimes is None else len(regimes)))
    first = regimes[0]
    if not torch.is_tensor(first) or first.dim() != 2:
        raise ValueError("{}: regimes[0] must be a [batch_size, num_trajectories] int32 tensor".format(name))
    shape = (batch_size, first.size(1))
    for time, regime in enumerate(regimes):
        if not torch.is_tensor(regime) or tuple(regime.shape) != shape or regime.dtype != torch.int32 or \
                regime.device != device:
            raise ValueError("{}: regimes[{}] must be {} int32 on {}".format(name, time, shape, device))
    return shape[1]


def _conditional_filter(provider, ops, observations, regimes, num_regimes, mask):
    """(means, covariances, log_likelihood, whether a regime was out of range: a device flag) of K31 forced along `regimes`
    — `testing.rao_blackwell._forced`: every cumulative row (1/M, .., 1), the uniform (s + 1/2) / M, no ancestors; `mask`:
    `_observed_steps`'s.  Reads no flags and nothing else from the device."""
    device = regimes[0].device
    edges = (torch.arange(num_regimes, dtype=torch.float64, device=device) + 1.0) / num_regimes
    forced = dict(ops, cdf0=edges, cdf=edges.expand(num_regimes, num_regimes).contiguous())
    log_likelihood = torch.zeros(regimes[0].shape, dtype=torch.float64, device=device)
    outside = torch.zeros((), dtype=torch.bool, device=device)
    means, covariances, state = [], [], None
    for time, (regime, observation) in enumerate(zip(regimes, observations)):
        outside = outside | ((regime < 0) | (regime >= num_regimes)).any()
        uniforms = (regime.to(torch.float64) + 0.5) / num_regimes
        drawn, mean, cov, log_w = provider.switching_kalman_step(forced, state, None, uniforms, observation, **mask(time))
        state = (drawn, mean, cov)
        log_likelihood = log_likelihood + log_w
        means.append(mean), covariances.append(cov)
    return means, covariances, log_likelihood, outside


def _finish_conditional(name, provider, device, outside, log_likelihood):
    """The one read at the end of a run along given regimes: the flags, the out-of-range marker, the NaN check."""
    flags = provider.read_flags(device)
    if bool(outside):
        raise ValueError("{}: regimes holds a value outside [0, M)".format(name))
    inference._raise_for_flags(flags)
    if bool(torch.isnan(log_likelihood).any()):
        raise FloatingPointError("log_weight contains nan element(s)")


def _prepare_conditional(name, provider, observations, model, regimes, observed):
    num_timesteps = len(observations)
    if num_timesteps == 0:
        raise ValueError("{}: observations must hold at least one timestep".format(name))
    ops = model.operands()
    num_trajectories = regimes[0].size(1) if regimes is not None and len(regimes) and torch.is_tensor(regimes[0]) and \
        regimes[0].dim() == 2 else 1
    batch_size, device = _check_observations(name, provider, observations, model, num_trajectories)
    num_trajectories = _check_regimes(name, regimes, num_timesteps, batch_size, device)
    if batch_size * num_trajectories > 0x7fffffff // (MAX_LATENT_DIM * MAX_LATENT_DIM):
        _refuse("{} trajectories in {} batch rows (batch_size * num_trajectories * D^2 beyond 32-bit element arithmetic)"
                .format(num_trajectories, batch_size))
    return ops, num_timesteps, batch_size, num_trajectories, device, _observed_steps(name, observed, observations)


def conditional_kalman_filter(observations, model, regimes, observed=None):
    """The exact Kalman filter of z given a regime path per trajectory: K31 with the regime FORCED (every cumulative row
    replaced by (1/M, .., 1) and the uniform by (s + 1/2) / M), no ancestors, one particle per trajectory.

    observations, model, observed: as `switching_filter`'s.  regimes: T int32 [batch_size, N] tensors on the device — what
    `switching_backward_simulate` returns, or any paths of the caller's.

    Returns a dict: means (T float64 [batch_size, N, D]), covariances (T float64 [batch_size, N, D(D+1)/2], packed) — the
    moments of p(z_t | y_{0:t}, s_{0:t}) — and log_likelihood [batch_size, N] float64: log p(y_{0:T-1} | s_{0:T-1}), the sum of
    the steps' log-weights.

    ValueError for an invalid model, T == 0, regimes of the wrong length, shape or dtype, and — read once, at the end, with
    the flags — a regime outside [0, M) (a forced uniform built from one would draw a wrong regime silently).  Refusals,
    flags and NaNs as `switching_filter`'s; an exception on the way discards whatever was flagged.  No host synchronisation
    inside the loop.  N == 0 gives empty tensors without a launch.  Runs under torch.no_grad(): NOT differentiable."""
    name = "conditional_kalman_filter"
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops, num_timesteps, batch_size, num_trajectories, device, mask = _prepare_conditional(
                name, provider, observations, model, regimes, observed)
            D = model.latent_dim
            if num_trajectories == 0:
                empty = lambda *tail: torch.empty((batch_size, 0) + tail, dtype=torch.float64, device=device)
                return {"means": [empty(D) for _ in range(num_timesteps)],
                        "covariances": [empty(D * (D + 1) // 2) for _ in range(num_timesteps)], "log_likelihood": empty()}
            means, covariances, log_likelihood, outside = _conditional_filter(provider, ops, observations, regimes,
                                                                              model.num_regimes, mask)
            _finish_conditional(name, provider, device, outside, log_likelihood)
    except BaseException:
        inference._discard_pending_flags()
        raise
    return {"means": means, "covariances": covariances, "log_likelihood": log_likelihood}


def switching_state_smooth(observations, model, regimes, return_cross_moments=False, return_trajectories=False,
                           observed=None):
    """The smoothed continuous state of a `SwitchingLinearGaussian` from regime trajectories: along a trajectory the model is
    linear-Gaussian and its smoother exact, and the estimate is the average of those exact smoothers over the trajectories
    (Fong, Godsill, Doucet & West 2002; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016) — the regimes alone are sampled.

    observations, model, observed: as `switching_filter`'s.  regimes: T int32 [batch_size, N] on the device: equally weighted
    trajectories, `switching_backward_simulate`'s (or any paths: the result is then the exact smoother given them).

    `conditional_kalman_filter` runs forward; for t = T-2 .. 0 K34 takes the trajectory's information one step back under its
    regime at t+1 and K36 (`aesmc_switching_smooth_combine`) combines it with the filter's moments of time t — the two-filter
    form, which factors I + F^T P F (pivots at least 1) and never the predicted covariance: models with q = 0 components
    and P = 0 are fine.  At T-1 the smoothed moments are the filtered ones.

    Returns a dict: smoothed_mean [T, batch_size, D] (the average over the N trajectories: the estimate of E[z_t | y_{0:T-1}]);
    smoothed_covariance [T, batch_size, D, D] (the mixture's, mean(P^s + m^s m^sT) - mean mean^T: of Cov[z_t | y_{0:T-1}]);
    log_likelihood [batch_size, N] (`conditional_kalman_filter`'s).  With return_cross_moments, smoothed_cross_moment
    [T-1, batch_size, D, D]: mean_n(cross_n + m^s_{t+1,n} m^sT_{t,n}), the estimate of E[z_{t+1} z_t^T | y_{0:T-1}] (rows: t+1)
    — what an EM M-step for A, b, q needs.  With return_trajectories, the per-trajectory means (T [batch_size, N, D]),
    covariances (T [batch_size, N, D(D+1)/2], packed) and cross_covariances (T-1 [batch_size, N, D, D]: Cov(z_{t+1,i},
    z_{t,l} | y, s)).  The cross-covariances are asked of K36 only with one of the two.

    Validation, refusals and flags as `conditional_kalman_filter`'s: one read at the end, an exception on the way discards
    whatever was flagged, no host synchronisation inside the loops.  N == 0 gives zero moments and empty trajectories
    without a launch; T == 1 launches no K34 and no K36.  Runs under torch.no_grad(): NOT differentiable."""
    name = "switching_state_smooth"
    provider = _kernels.get()
    want_cross = bool(return_cross_moments or return_trajectories)
    try:
        with torch.no_grad(), _syncfree.scope():
            ops, num_timesteps, batch_size, num_trajectories, device, mask = _prepare_conditional(
                name, provider, observations, model, regimes, observed)
            D = model.latent_dim
            last = num_timesteps - 1
            if num_trajectories == 0:
                zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=device)
                empty = lambda *tail: torch.empty((batch_size, 0) + tail, dtype=torch.float64, device=device)
                out = {"smoothed_mean": zeros(num_timesteps, batch_size, D),
                       "smoothed_covariance": zeros(num_timesteps, batch_size, D, D), "log_likelihood": empty()}
                if return_cross_moments:
                    out["smoothed_cross_moment"] = zeros(last, batch_size, D, D)
                if return_trajectories:
                    out.update(means=[empty(D) for _ in range(num_timesteps)],
                               covariances=[empty(D * (D + 1) // 2) for _ in range(num_timesteps)],
                               cross_covariances=[empty(D, D) for _ in range(last)])
                return out
            filtered_means, filtered_covs, log_likelihood, outside = _conditional_filter(provider, ops, observations, regimes,
                                                                                         model.num_regimes, mask)
            means, covs, crosses = [None] * num_timesteps, [None] * num_timesteps, [None] * last
            means[last], covs[last] = filtered_means[last], filtered_covs[last]
            info = None
            for time in range(last - 1, -1, -1):
                omega_next = None if info is None else info[0]
                omega, lam, c, factor = provider.switching_information_step(ops, regimes[time + 1], info,
                                                                            observations[time + 1], **mask(time + 1))
                info = (omega, lam, c)
                if want_cross:
                    # (K36 adds the information of y_{t+1} to Om_{t+1}: under a mask only its observed components', K42)
                    seen = {"observed_next": mask(time + 1)["observed"]} if mask(time + 1) else {}
                    means[time], covs[time], crosses[time] = provider.switching_smooth_combine(
                        ops, regimes[time + 1], (filtered_means[time], filtered_covs[time]), factor, lam, omega_next,
                        covs[time + 1], **seen)
                else:
                    means[time], covs[time], _ = provider.switching_smooth_combine(
                        None, None, (filtered_means[time], filtered_covs[time]), factor, lam)
            stacked = torch.stack(means)                                                   # [T,B,N,D]
            average = stacked.mean(dim=2)
            second = (unpack_covariance(torch.stack(covs), D) + stacked.unsqueeze(-1) * stacked.unsqueeze(-2)).mean(dim=2)
            out = {"smoothed_mean": average,
                   "smoothed_covariance": second - average.unsqueeze(-1) * average.unsqueeze(-2),
                   "log_likelihood": log_likelihood}
            if return_cross_moments:
                out["smoothed_cross_moment"] = (torch.stack(crosses) + stacked[1:].unsqueeze(-1) *
                                                stacked[:-1].unsqueeze(-2)).mean(dim=2) if last > 0 else \
                    torch.zeros((0, batch_size, D, D), dtype=torch.float64, device=device)
            if return_trajectories:
                out.update(means=means, covariances=covs, cross_covariances=crosses)
            _finish_conditional(name, provider, device, outside, log_likelihood)
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


def _state_noise(name, noise, num_timesteps, shape, device):
    """The T standard-normal tensors of a state draw: fresh from torch's device generator, or the replayed ones, validated."""
    from . import distributed
    if noise is None:
        if distributed.active_shard() is not None:
            raise NotImplementedError(
                "aesmc_amd.rao_blackwell: drawing the state noise inside distributed.shard_scope is not implemented: a "
                "sharded run reproduces the unsharded one through the global block of host uniforms every rank draws, which "
                "per-trajectory device draws do not have. Pass noise when sharding.")
        return None
    try:
        length = len(noise)
    except TypeError:
        length = -1
    if length != num_timesteps:
        raise ValueError("{}: noise must be None or hold one tensor per timestep ({}), got {}".format(
            name, num_timesteps, "{} entries".format(length) if length >= 0 else type(noise).__name__))
    for time in range(length):
        eps = noise[time]
        if not torch.is_tensor(eps) or tuple(eps.shape) != shape or eps.dtype != torch.float64 or eps.device != device:
            raise ValueError("{}: noise[{}] must be {} float64 on {}".format(name, time, shape, device))
    return list(noise)


def switching_sample_states(observations, model, regimes, noise=None, observed=None):
    """A draw of the continuous state along given regime paths: z_{0:T-1} ~ p(z | s_{0:T-1}, y) per trajectory, by forward
    filtering and backward sampling (Fruehwirth-Schnatter 1994; Carter & Kohn 1994) — the simulation smoother.  With
    `switching_particle_gibbs` for (s | theta, y) and conjugate draws for (theta | s, z, y) it is the middle block of a Gibbs
    sampler over regimes, states and every parameter (examples/slds_gibbs_full.py); the draws also give posterior samples of
    any nonlinear functional of the state path (maxima, threshold crossings), which the two moments of
    `switching_state_smooth` cannot.

    observations, model, observed: as `switching_filter`'s (`observed` reaches the filter only: missing observations are in
    the filtered moments, the backward pass reads no y).  regimes: T int32 [batch_size, N] on the device, as
    `conditional_kalman_filter`'s.  noise: None — torch.randn float64 on the device (refused inside
    distributed.shard_scope) — or a length-T sequence of float64 [batch_size, N, D] standard normals on the device, for replay.

    `conditional_kalman_filter`'s loop runs forward; then one torch.stack per operand and ONE launch of K47
    (`aesmc_switching_state_draw`) walk every trajectory from T-1 to 0: a Kalman measurement update of N(m_t, P_t) by
    z_{t+1} through A, b, q of s_{t+1}, then z_t = m' + chol(P') eps_t.  Both factorisations drop a pivot at or below 2^-40
    of the largest diagonal entry: q = 0 components and P = 0 are fine.  T == 1 is the draw from the filtered law.

    Returns a dict: states (T float64 [batch_size, N, D], views of one tensor), log_likelihood [batch_size, N] (the
    conditional filter's log p(y | s_{0:T-1})) and noise (the T tensors that were used).

    Validation, refusals and flags as `conditional_kalman_filter`'s: one read at the end, an exception on the way discards
    whatever was flagged, no host synchronisation before that read.  N == 0 gives empty tensors without a launch.  Runs
    under torch.no_grad(): NOT differentiable."""
    name = "switching_sample_states"
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops, num_timesteps, batch_size, num_trajectories, device, mask = _prepare_conditional(
                name, provider, observations, model, regimes, observed)
            D = model.latent_dim
            shape = (batch_size, num_trajectories, D)
            noise = _state_noise(name, noise, num_timesteps, shape, device)
            if num_trajectories == 0:
                empty = lambda *tail: torch.empty((batch_size, 0) + tail, dtype=torch.float64, device=device)
                return {"states": [empty(D) for _ in range(num_timesteps)], "log_likelihood": empty(),
                        "noise": [empty(D) for _ in range(num_timesteps)] if noise is None else noise}
            means, covariances, log_likelihood, outside = _conditional_filter(provider, ops, observations, regimes,
                                                                              model.num_regimes, mask)
            stacked_noise = torch.randn((num_timesteps,) + shape, dtype=torch.float64, device=device) if noise is None else \
                torch.stack(noise)
            states = provider.switching_state_draw(ops, torch.stack(list(regimes)), torch.stack(means),
                                                   torch.stack(covariances), stacked_noise)
            _finish_conditional(name, provider, device, outside, log_likelihood)
    except BaseException:
        inference._discard_pending_flags()
        raise
    return {"states": list(states.unbind(0)), "log_likelihood": log_likelihood,
            "noise": list(stacked_noise.unbind(0)) if noise is None else noise}


def _collapsed_forward(provider, ops, observations, num_regimes, order, mask, log_priors=None):
    """The forward pass of the collapsed-mixture filters (`testing.switching_collapsed.collapsed_pass`, call for call): per
    step K31 forced (`_conditional_filter`'s shim) on M^2 pair slots (order 2) or M slots (order 1, and step 0), K50 over the
    pairs or the mixing weights, and K50 once more over the M components for the increment and the overall moments.  Returns
    a dict of T-lists: log_mu [B,M], means [B,M,D], covariances [B,M,TD], scores ([B,M,M] indexed (b,j,i), order 2, t >= 1;
    else None), masses ([B,M]; None at step 0), increments [B], overall_mean [B,D], overall_cov [B,TD].  Reads nothing from
    the device.  log_priors: (log pi0, log Pi) where the caller forms them itself (`collapsed_switching_log_likelihood`:
    with a zero gradient at a zero probability); None: torch.log of the operands."""
    M = num_regimes
    B, device = observations[0].size(0), observations[0].device
    edges = (torch.arange(M, dtype=torch.float64, device=device) + 1.0) / M
    forced = dict(ops, cdf0=edges, cdf=edges.expand(M, M).contiguous())
    # (-inf where a probability is 0) once
    log_pi0, log_Pi = (torch.log(ops["pi0"]), torch.log(ops["Pi"])) if log_priors is None else log_priors
    transposed = log_Pi.t().unsqueeze(0)                                # [1,j,i] = log Pi[i,j]
    slots = torch.arange(M, dtype=torch.int32, device=device).expand(B, M).contiguous()
    slot_uniforms = (slots.to(torch.float64) + 0.5) / M
    pair_slots = slots.repeat(1, M)                                     # slot j M + i: component i ...
    pair_uniforms = slot_uniforms.repeat_interleave(M, dim=1)           # ... under regime j
    # a score whose prior part is -inf is -inf whatever its likelihood part is (K32's rule)
    scored = lambda prior, likelihood: torch.where(prior == -math.inf, prior, prior + likelihood)
    out = {name: [] for name in ("log_mu", "means", "covariances", "scores", "masses", "increments", "overall_mean",
                                 "overall_cov")}
    log_mu = mean = cov = None
    for time, observation in enumerate(observations):
        scores = mass = None
        if time == 0:
            _, mean, cov, likelihood = provider.switching_kalman_step(forced, None, None, slot_uniforms, observation, **mask(0))
            g = scored(log_pi0.expand(B, M), likelihood)
        else:
            prior = log_mu.unsqueeze(1) + transposed                    # [b,j,i] = log mu_i + log Pi[i,j]
            if order == 2:
                state = (pair_slots, mean.repeat(1, M, 1), cov.repeat(1, M, 1))
                _, pair_mean, pair_cov, likelihood = provider.switching_kalman_step(forced, state, None, pair_uniforms,
                                                                                    observation, **mask(time))
                scores = scored(prior, likelihood.reshape(B, M, M))
                mass, mean, cov = provider.switching_collapse(pair_mean.reshape(B, M, M, -1), pair_cov.reshape(B, M, M, -1),
                                                              scores)
                g = mass
            else:
                mass, mixed_mean, mixed_cov = provider.switching_collapse(mean, cov, prior)      # (the shared-components form)
                _, mean, cov, likelihood = provider.switching_kalman_step(forced, (slots, mixed_mean, mixed_cov), None,
                                                                          slot_uniforms, observation, **mask(time))
                g = scored(mass, likelihood)
        increment, overall_mean, overall_cov = provider.switching_collapse(mean.unsqueeze(1), cov.unsqueeze(1), g.unsqueeze(1))
        log_mu = g - increment
        for name, value in (("log_mu", log_mu), ("means", mean), ("covariances", cov), ("scores", scores), ("masses", mass),
                            ("increments", increment.squeeze(1)), ("overall_mean", overall_mean.squeeze(1)),
                            ("overall_cov", overall_cov.squeeze(1))):
            out[name].append(value)
    return out


def _prepare_collapsed(name, provider, observations, model, slots_per_regime, observed):
    if len(observations) == 0:
        raise ValueError("{}: observations must hold at least one timestep".format(name))
    ops = model.operands()
    _, device = _check_observations(name, provider, observations, model, model.num_regimes * slots_per_regime)
    return ops, device, _observed_steps(name, observed, observations)


def _collapsed_filter_results(forward, D, return_components):
    total = forward["increments"][0]
    for increment in forward["increments"][1:]:
        total = total + increment
    out = {"log_marginal_likelihood": total, "regime_probabilities": torch.exp(torch.stack(forward["log_mu"])),
           "filtered_mean": torch.stack(forward["overall_mean"]),
           "filtered_covariance": unpack_covariance(torch.stack(forward["overall_cov"]), D)}
    if return_components:
        out.update(log_regime_probabilities=forward["log_mu"], means=forward["means"], covariances=forward["covariances"])
    return out


def collapsed_switching_filter(observations, model, order=2, observed=None, return_components=False):
    """The deterministic collapsed-mixture filter of a `SwitchingLinearGaussian`: GPB2, which is Kim's filter (Kim 1994; Kim &
    Nelson 1999), for order=2, and its first-order cousin IMM (Blom & Bar-Shalom 1988) for order=1.  No particles and no
    random numbers: per series M Gaussians (log mu_i, m_i, P_i), mu_i = p(s_t = i | y_{0:t}), and M^2 (order 1: M) Kalman
    updates per step where a particle filter makes K M.  What the particle filters of this module are held against: a fast,
    noise-free approximate evidence and segmentation of thousands of series — a likelihood surface, a start for EM or Gibbs
    (examples/slds_gibbs.py --start collapsed), a sanity check of a particle run (examples/slds_filter.py --collapsed).

    observations, model, observed: as `switching_filter`'s (`observed` reaches K31's masked entry K39 unchanged; K50 reads no
    y).  order: 2 or 1.

    Step 0: K31's step-0 form on M slots, slot j forced to regime j as `conditional_kalman_filter` forces it: (m_j, P_j,
    l_j), g_j = log pi0_j + l_j.  Order 2, t >= 1: K31 forced on M^2 pair slots (slot j M + i: component i under regime j),
    g[b,j,i] = log mu_i + log Pi[i,j] + l_ij, and K50 (`aesmc_switching_collapse`, the moment-matching collapse) of every
    group j over i: (mass_j, m_j, P_j), g_j = mass_j.  Order 1, t >= 1: K50 in its shared-components form mixes the M
    components once per target regime j under log mu_i + log Pi[i,j]: (log c_j, m0_j, P0_j); K31 forced on M slots from
    those: g_j = log c_j + l_j.  Every step: K50 over the one group of the M components under g — its mass is the evidence
    increment lse_j g_j, its mean and covariance the filtered ones — and log mu_j = g_j - increment.  Everything stays in the
    log domain; a score whose prior part is -inf is -inf whatever its likelihood part is (K32's rule: a singular innovation
    under an impossible regime is ignored).

    Returns a dict: log_marginal_likelihood [batch_size] float64 — DETERMINISTIC and APPROXIMATE: the sum of the
    increments, not an unbiased estimate and not a bound.  It is exact (to rounding) for order 2 while T <= 2, for order 1 at
    T = 1, and for both orders and any T with one regime or with dynamics and emission shared across regimes; otherwise off by
    the moment matching (DESIGN 30 has figures: a few 1e-3 for order 2, a few 1e-2 for order 1 on this package's example
    models).  regime_probabilities [T, batch_size, M] (p(s_t | y_{0:t})), filtered_mean [T, batch_size, D] and
    filtered_covariance [T, batch_size, D, D] (the moments of the M-component mixture).  With return_components, T-lists of
    log_regime_probabilities [batch_size, M], means [batch_size, M, D] and covariances [batch_size, M, D(D+1)/2] (packed);
    the moments of a regime of probability zero are whatever K31 or K50 left there and are read by nothing.

    ValueError for an invalid model, T == 0 and an order that is not 1 or 2.  Refusals, flags and NaNs as
    `conditional_kalman_filter`'s: read once, at the end; an exception on the way discards whatever was flagged.  No host
    synchronisation inside the loop.  Runs under torch.no_grad(): NOT differentiable."""
    name = "collapsed_switching_filter"
    if order not in (1, 2):
        raise ValueError("{}: order must be 1 or 2, got {!r}".format(name, order))
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops, device, mask = _prepare_collapsed(name, provider, observations, model,
                                                   model.num_regimes if order == 2 else 1, observed)
            forward = _collapsed_forward(provider, ops, observations, model.num_regimes, order, mask)
            out = _collapsed_filter_results(forward, model.latent_dim, return_components)
            _finish_conditional(name, provider, device, False, out["log_marginal_likelihood"])
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


class _DifferentiableSteps:
    """What `_collapsed_forward` asks of a provider, answered by the autograd functions of `_ops` around the same provider
    calls (K31 forced and K50 forward, K52 / K53 and K54 backward)."""

    @staticmethod
    def switching_kalman_step(model, state, index, uniforms, observation, observed=None):
        assert index is None
        return _ops.switching_kalman_step_forced(model, state, uniforms, observation, observed)

    @staticmethod
    def switching_collapse(means, covs, log_weights):
        return _ops.switching_collapse(means, covs, log_weights)


def _log_probabilities(probabilities):
    """log p, -inf where p is exactly 0, with a gradient of exactly 0 there: a zero probability is structural (torch.log's
    backward forms 0 / 0 = NaN at such an entry)."""
    positive = probabilities > 0
    return torch.where(positive, torch.log(torch.where(positive, probabilities, torch.ones_like(probabilities))),
                       torch.full_like(probabilities, -math.inf))


def collapsed_switching_log_likelihood(observations, parameters, order=2, observed=None):
    """The log-evidence of `collapsed_switching_filter` WITH its graph: float64 [batch_size], differentiable in the ten
    parameters of the model — the one differentiable function of this module.  The collapsed-mixture filter is
    deterministic (no particles, no random numbers, no resampling), so this is the exact gradient of a deterministic,
    approximate objective: no genealogy bias and no score-function term.

    parameters: a mapping with the ten names of `PARAMETERS` to float64 tensors on the observations' device, any of which
    may require grad, in the shapes `SwitchingLinearGaussian` takes (a leading 1 for parameters shared across regimes, one
    value or D for s0) — the user's own parametrisation (softmax rows, exp of log-scales, the output of a network) stays
    in torch ops in front of it (examples/slds_sgd.py).  A `SwitchingLinearGaussian` is accepted too and gives a result
    without a graph.  observations, order, observed: as `collapsed_switching_filter`'s.

    The pass is `collapsed_switching_filter`'s, call for call, with autograd enabled: K31 forced (masked: K39) and K50 run
    as there, and the value is `torch.equal` to its log_marginal_likelihood; backwards each call is one launch of its
    adjoint — K52 (K53) `aesmc_switching_kalman_step_backward` with its finishing launch, K54
    `aesmc_switching_collapse_backward` — which recompute the forward chains (nothing but the calls' inputs is kept) and
    compute only what `needs_input_grad` asks for.  Shared or expanded parameters get their sums from `expand`'s own
    backward.  Gradients are with respect to q, r and s0 themselves.  A probability that is exactly 0 in pi0 or Pi is
    structural: its gradient is exactly 0 and every other gradient stays finite.  First order only.

    Validation goes through `SwitchingLinearGaussian(...).operands()` on detached values (the same errors, one host copy);
    flags and the NaN check are read once at the end of the forward, as the filter's.  NotImplementedError during a
    hipGraph capture and inside `distributed.shard_scope`."""
    from . import distributed
    name = "collapsed_switching_log_likelihood"
    if order not in (1, 2):
        raise ValueError("{}: order must be 1 or 2, got {!r}".format(name, order))
    if distributed.active_shard() is not None:
        raise NotImplementedError("aesmc_amd.rao_blackwell: {} inside distributed.shard_scope is not implemented".format(name))
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise NotImplementedError("aesmc_amd.rao_blackwell: {} cannot be captured into a hipGraph (its backward allocates "
                                  "per call and the flags are read back)".format(name))
    if isinstance(parameters, SwitchingLinearGaussian):
        model = parameters
        given = {key: getattr(model, key) for key in PARAMETERS}
    else:
        try:
            given = {key: parameters[key] for key in PARAMETERS}
        except (KeyError, TypeError, IndexError):
            raise ValueError("{}: parameters must be a SwitchingLinearGaussian or a mapping with the keys {}".format(
                name, ", ".join(PARAMETERS)))
        for key, value in given.items():
            if not torch.is_tensor(value) or value.dtype != torch.float64:
                raise ValueError("{}: parameters[{!r}] must be a float64 tensor, got {}".format(
                    name, key, value.dtype if torch.is_tensor(value) else type(value).__name__))
        model = SwitchingLinearGaussian(**{key: value.detach() for key, value in given.items()})
    provider = _kernels.get()
    try:
        with _syncfree.scope():
            with torch.no_grad():
                checked, device, mask = _prepare_collapsed(name, provider, observations, model,
                                                           model.num_regimes if order == 2 else 1, observed)
            for key, value in given.items():
                if value.device != device:
                    raise ValueError("{}: parameters[{!r}] is on {}, the observations on {}".format(name, key, value.device,
                                                                                                  device))
            # the validated operands, rebuilt from the given tensors so that the graph reaches them: the same values
            ops = {key: given[key].reshape(-1).expand(checked[key].shape).contiguous() if key == "s0" else
                   given[key].expand(checked[key].shape).contiguous() for key in PARAMETERS}
            ops.update(cdf0=checked["cdf0"], cdf=checked["cdf"])
            forward = _collapsed_forward(_DifferentiableSteps, ops, observations, model.num_regimes, order, mask,
                                         log_priors=(_log_probabilities(ops["pi0"]), _log_probabilities(ops["Pi"])))
            total = forward["increments"][0]
            for increment in forward["increments"][1:]:
                total = total + increment
            _finish_conditional(name, provider, device, False, total.detach())
    except BaseException:
        inference._discard_pending_flags()
        raise
    return total


def collapsed_switching_loss(observations, parameters, order=2, observed=None):
    """Minus the batch mean of `collapsed_switching_log_likelihood`: a scalar to minimise."""
    return -collapsed_switching_log_likelihood(observations, parameters, order=order, observed=observed).mean()


def collapsed_switching_smooth(observations, model, observed=None):
    """The collapsed-mixture smoother (Kim 1994; Kim & Nelson 1999) of a `SwitchingLinearGaussian`: `collapsed_switching_filter`
    of order 2, keeping each step's pair scores g_t and masses, then backwards for t = T-2 .. 0:

        log joint[b,i,j] = (g_{t+1}[b,j,i] - mass_{t+1}[b,j]) + log mu^s_{t+1}[b,j]

    (the first term is p(s_t = i | s_{t+1} = j, y_{0:t+1}), one observation more than Kim's original uses); K51
    (`aesmc_switching_pair_smooth`, a Rauch-Tung-Striebel step between components) forms the pair-smoothed (m_ij, P_ij) from
    component i filtered at t and regime j's smoothed component of t+1; K50 collapses group i over j under log joint[b,i,:]
    — its mass is log mu^s_t(i) — and once more the M smoothed components into the smoothed moments.  At T-1 the smoothed
    quantities are the filtered ones.  K51 drops pivots as K47 does: q = 0 components and P = 0 are fine.

    observations, model, observed: as `collapsed_switching_filter`'s.  Returns its keys (without components) plus
    smoothed_regime_probabilities [T, batch_size, M] (p(s_t | y_{0:T-1})), smoothed_pair_probabilities [T-1, batch_size, M, M]
    (p(s_t = i, s_{t+1} = j | y_{0:T-1}), indexed (i, j)), smoothed_mean [T, batch_size, D] and smoothed_covariance
    [T, batch_size, D, D].  All approximate, by the same moment matching; exact (to rounding) for the regime probabilities
    at T = 2, and for everything with one regime or with dynamics and emission shared across regimes.  Deterministic: a start
    for `switching_particle_gibbs` is the argmax of smoothed_regime_probabilities.

    Validation, refusals, flags and NaNs as `collapsed_switching_filter`'s: one read at the end, no host synchronisation
    inside the loops.  Runs under torch.no_grad(): NOT differentiable."""
    name = "collapsed_switching_smooth"
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops, device, mask = _prepare_collapsed(name, provider, observations, model, model.num_regimes, observed)
            M, D = model.num_regimes, model.latent_dim
            forward = _collapsed_forward(provider, ops, observations, M, 2, mask)
            out = _collapsed_filter_results(forward, D, False)
            last = len(observations) - 1
            log_s, mean, cov = forward["log_mu"][last], forward["means"][last], forward["covariances"][last]
            regimes, pairs = [None] * last + [log_s], [None] * last
            centre, spread = [None] * last + [forward["overall_mean"][last]], [None] * last + [forward["overall_cov"][last]]
            for time in range(last - 1, -1, -1):
                conditional = (forward["scores"][time + 1] - forward["masses"][time + 1].unsqueeze(2)).transpose(1, 2)
                prior = log_s.unsqueeze(1)                              # [b,i,j]: log mu^s_{t+1}(j)
                joint = torch.where(prior == -math.inf, prior, conditional + prior)
                pair_mean, pair_cov = provider.switching_pair_smooth(ops, forward["means"][time], forward["covariances"][time],
                                                                     mean, cov)
                log_s, mean, cov = provider.switching_collapse(pair_mean, pair_cov, joint)
                _, overall_mean, overall_cov = provider.switching_collapse(mean.unsqueeze(1), cov.unsqueeze(1),
                                                                           log_s.unsqueeze(1))
                regimes[time], pairs[time] = log_s, joint
                centre[time], spread[time] = overall_mean.squeeze(1), overall_cov.squeeze(1)
            batch_size = observations[0].size(0)
            out.update(smoothed_regime_probabilities=torch.exp(torch.stack(regimes)),
                       smoothed_pair_probabilities=torch.exp(torch.stack(pairs)) if last > 0 else
                       torch.zeros((0, batch_size, M, M), dtype=torch.float64, device=device),
                       smoothed_mean=torch.stack(centre), smoothed_covariance=unpack_covariance(torch.stack(spread), D))
            _finish_conditional(name, provider, device, False, out["log_marginal_likelihood"])
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


def switching_smooth_states(observations, model, num_particles, num_trajectories=None, resampling=None, lookahead=False,
                            return_trajectories=False, observed=None):
    """Runs `switching_filter` (lookahead: `adapted_switching_filter`), `switching_backward_simulate` over what it stored and
    `switching_state_smooth` along the drawn trajectories with return_cross_moments (K34 runs once more along the drawn
    regimes: B N lanes, a tenth of a backward step).  Returns (a dict: `switching_backward_simulate`'s regimes and
    smoothed_regime_probabilities with `switching_state_smooth`'s smoothed_mean, smoothed_covariance, smoothed_cross_moment
    and log_likelihood — with return_trajectories its per-trajectory means, covariances and cross_covariances too —, the
    filter's log_marginal_likelihood [batch_size]).  `observed` (`switching_filter`'s) goes to all three."""
    run = adapted_switching_filter if lookahead else switching_filter
    filtered = run(observations, model, num_particles, resampling=resampling, observed=observed)
    out = switching_backward_simulate(filtered, model, observations, num_trajectories=num_trajectories, observed=observed)
    out.update(switching_state_smooth(observations, model, out["regimes"], return_cross_moments=True,
                                      return_trajectories=return_trajectories, observed=observed))
    return out, filtered["log_marginal_likelihood"]


def conditional_switching_filter(observations, model, num_particles, reference, ancestor_sampling=True, uniforms=None,
                                 regime_uniforms=None, return_particles=False, observed=None, lookahead=False):
    """One sweep of particle Gibbs on the regimes of a `SwitchingLinearGaussian`: a Rao-Blackwellised conditional particle
    filter whose slot num_particles - 1 carries the regime path `reference`, then one draw of a path from the final weights
    along the ancestors.  The kernel leaves p(s_{0:T-1} | y_{0:T-1}) invariant for ANY number of particles (Andrieu, Doucet &
    Holenstein 2010; with z integrated out: Whiteley, Andrieu & Doucet 2010).

    observations, model, num_particles: as `switching_filter`'s.
    reference: T int32 [batch_size] tensors on the device, one regime path per batch row.
    ancestor_sampling: True — backwards first: for t = T-1 .. 1 the information step K34 along the reference (one trajectory
        per row) stores (F, lam) per step; going forwards, the pinned slot's ancestor at step t is drawn in proportion to
        weight x Pi[s, reference[t]] x the closed-form integral of the reference's future against the stored particle's
        N(m, P) (K35's score; Lindsten, Bunch, Saerkkae, Schoen & Godsill 2016).  False — the pinned slot keeps ancestor
        num_particles - 1 and no backward pass runs.
    uniforms: `particle_gibbs.conditional_smc`'s convention — None: fresh float64 blocks from torch's generator for the
        device (seed with torch.manual_seed); or a length-T sequence: `uniforms[t]` [batch_size, num_particles] for t <=
        T-2 — the ancestors of step t+1, from step t's weights (column k is slot k's) — and `uniforms[T-1]` [batch_size, 1]
        for the final draw (replay).
    regime_uniforms: None, or T float64 [batch_size, num_particles] tensors: the regime draws of every step (column
        num_particles - 1 is not used: that slot's regime is the reference's).
        Fresh blocks are drawn in this order: step 0's regime block; then per step t = 1 .. T-1 the resampling block
        `uniforms[t-1]` and the step's regime block; last the [batch_size, 1] block of the final draw.  Inside
        `distributed.shard_scope` a None of either raises NotImplementedError, as `switching_filter`'s does.
    return_particles: also a dict with the stored systems — regimes (T int32 [batch_size, K], the reference in slot K-1),
        means, covariances (packed), log_weights — and ancestral_indices ((T-1) int64 [batch_size, K]) and indices (T int64
        [batch_size]: the slot the new path passes through).
    observed: `switching_filter`'s (K41 along the reference, K39 with the pinned regime in place of K38).
    lookahead: False — the sweep described here, call for call.  True — the look-ahead (fully adapted) conditional filter:
        the free slots resample on the exact first-stage weights p(y_t | history) of the stored system and draw the regime
        from the ANCESTOR'S exact posterior row, as `adapted_switching_filter` does; slot num_particles - 1 takes the
        reference's regime.  Every stored system is then equally weighted, so the pinned slot's ancestor is drawn in
        proportion to Pi[s, reference[t]] x K35's integral alone — it does NOT carry the first-stage weight — and the final
        draw is from equal weights.  Step 0 is K32 on the prior and the step; a later step is K48
        (`aesmc_switching_lookahead_conditional_ancestor_index`: the look-ahead and the conditional ancestors in one launch;
        past `switching_lookahead_conditional_max_particles` the provider composes it from K32 and K37) and K49
        (`aesmc_switching_kalman_conditional_draw`: K31 drawing from the ancestor's row with slot K-1 pinned).  The uniforms,
        their order and the limits are the same.  With return_particles, `log_weights` holds T zero tensors and
        `first_stage_log_weights` (T float64 [batch_size, K]; step 0's on the prior) is added.  With few particles a free
        slot meets a regime change in the step where it happens instead of only when it draws it from Pi.

    Returns T int32 [batch_size] tensors, the new path.  With return_particles: (path, particles).

    Per step one launch of K37 (`aesmc_switching_conditional_ancestor_index`: the K-1 free multinomial ancestors and the
    pinned slot's in one go) and one of K38 (`aesmc_switching_kalman_conditional_step`: K31 with slot K-1's regime pinned);
    every slot, the pinned one included, is weighted by its Kalman predictive likelihood.  At the end one K21 draw per row and
    the walk back.  A sweep costs O(K) per step.

    ValueError for an invalid model, T == 0, K < 1, a reference, uniforms or regime_uniforms of the wrong length, shape or
    dtype; NotImplementedError naming the covered class past the limits (K above 8192, above 4096 for a latent of more than
    4 values).  NaN weights or scores raise FloatingPointError, a regime outside [0, M) and a row without a finite maximum
    (also: no stored particle can precede the reference) RuntimeError — read once, at the end; an exception on
    the way discards whatever was flagged.  No host synchronisation inside the loops.  Runs under torch.no_grad()."""
    name = "conditional_switching_filter"
    num_timesteps, num_particles = len(observations), int(num_particles)
    if num_timesteps == 0:
        raise ValueError("{}: observations must hold at least one timestep".format(name))
    if num_particles < 1:
        raise ValueError("{}: num_particles must be at least 1".format(name))
    if reference is None or len(reference) != num_timesteps:
        raise ValueError("{}: reference must hold one tensor per timestep ({}), got {}".format(
            name, num_timesteps, 0 if reference is None else len(reference)))
    for what, feed in (("uniforms", uniforms), ("regime_uniforms", regime_uniforms)):
        if feed is not None and len(feed) != num_timesteps:
            raise ValueError("{}: {} must hold one block per timestep ({}), got {}".format(name, what, num_timesteps,
                                                                                           len(feed)))
    if uniforms is None or regime_uniforms is None:
        from . import distributed
        if distributed.active_shard() is not None:
            raise NotImplementedError(
                "aesmc_amd.rao_blackwell: {} inside distributed.shard_scope draws its uniforms on the device, where no "
                "global block exists that every rank could cut its rows from. Pass uniforms= and regime_uniforms=."
                .format(name))
    provider = _kernels.get()
    pinned = num_particles - 1
    try:
        with torch.no_grad(), _syncfree.scope():
            ops = model.operands()
            M, D, Dy = model.num_regimes, model.latent_dim, model.observation_dim
            batch_size, device = _check_observations(name, provider, observations, model, num_particles)
            mask = _observed_steps(name, observed, observations)
            if not provider.switching_conditional_covers(observations[0], M, D, Dy, num_particles):
                _refuse("num_particles = {} with a latent of {} values (conditional resampling keeps its running sums in "
                        "LDS: at most 8192 particles, 4096 for a latent of more than 4 values)".format(num_particles, D))
            for time, regime in enumerate(reference):
                if not torch.is_tensor(regime) or tuple(regime.shape) != (batch_size,) or regime.dtype != torch.int32 or \
                        regime.device != device:
                    raise ValueError("{}: reference[{}] must be {} int32 on {}".format(name, time, (batch_size,), device))
            draw = _regime_draws(name, regime_uniforms, (batch_size, num_particles), device)

            def block(time):
                shape = (batch_size, 1 if time == num_timesteps - 1 else num_particles)
                if uniforms is None:
                    return torch.rand(shape, dtype=torch.float64, device=device)
                u = uniforms[time]
                if not torch.is_tensor(u) or tuple(u.shape) != shape or u.dtype != torch.float64 or u.device != device:
                    raise ValueError("{}: uniforms[{}] must be {} float64 on {}".format(name, time, shape, device))
                return u

            log_Pi = torch.log(ops["Pi"])      # (-inf where a probability is 0) once
            information = [None] * num_timesteps      # at position t: (F, lam) of the reference's future from t on
            if ancestor_sampling:
                info = None
                for time in range(num_timesteps - 1, 0, -1):
                    omega, lam, c, factor = provider.switching_information_step(ops, reference[time].unsqueeze(1), info,
                                                                                observations[time], **mask(time))
                    info = (omega, lam, c)
                    information[time] = (factor[:, 0], lam[:, 0])
            regimes, means, covariances, log_weights, ancestral, first_stage = [], [], [], [], [], []
            state, index = None, None
            for time in range(num_timesteps):
                if lookahead:
                    if time == 0:
                        regime_u = draw(0)
                        log_v, cdf = provider.switching_lookahead(ops, torch.log(ops["pi0"]), None, observations[0],
                                                                  num_particles=num_particles, **mask(0))
                    else:
                        factor, lam = information[time] if ancestor_sampling else (None, None)
                        resampling_u, regime_u = block(time - 1), draw(time)
                        index, log_v, cdf = provider.switching_lookahead_conditional_ancestor_index(
                            ops, log_Pi, state, observations[time], resampling_u, reference[time], factor, lam, **mask(time))
                        ancestral.append(index)
                        index = index.clamp(max=pinned)      # (a failed draw is position K, as below)
                    regime, mean, cov, _ = provider.switching_kalman_conditional_draw(ops, state, index, regime_u, cdf,
                                                                                      reference[time], observations[time],
                                                                                      **mask(time))
                    state = (regime, mean, cov)
                    regimes.append(regime), means.append(mean), covariances.append(cov), first_stage.append(log_v)
                    # the systems after a look-ahead draw are equally weighted: T zero tensors where they are returned, one
                    # for the final draw where they are not (a fill per step is a launch per step)
                    if return_particles or time == num_timesteps - 1:
                        log_weights.append(torch.zeros_like(log_v))
                    continue
                if time > 0:
                    factor, lam = information[time] if ancestor_sampling else (None, None)
                    index = provider.switching_conditional_ancestor_index(log_weights[-1], block(time - 1), log_Pi,
                                                                          reference[time], factor, lam, state)
                    ancestral.append(index)
                    # (a failed draw is position K: the step reads particle K-1 in its place, the flag raises at the end)
                    index = index.clamp(max=pinned)
                regime, mean, cov, log_w = provider.switching_kalman_conditional_step(ops, state, index, draw(time),
                                                                                      reference[time], observations[time],
                                                                                      **mask(time))
                state = (regime, mean, cov)
                regimes.append(regime), means.append(mean), covariances.append(cov), log_weights.append(log_w)
            last, _ = provider.backward_sample(log_weights[-1], None, None, None, block(num_timesteps - 1))
            indices = [None] * num_timesteps
            indices[-1] = last[:, 0]
            for time in range(num_timesteps - 2, -1, -1):
                # (an index of a flagged row is num_particles: the clamp keeps the read in range, the flag raises below)
                at = indices[time + 1].clamp(max=pinned).unsqueeze(1)
                indices[time] = torch.gather(ancestral[time], 1, at)[:, 0]
            path = [torch.gather(regimes[time], 1, indices[time].clamp(max=pinned).unsqueeze(1))[:, 0]
                    for time in range(num_timesteps)]
            inference._raise_for_flags(provider.read_flags(device))
            # (step 0's first-stage weights meet no resampling launch: a NaN among them is reported here, after the one read)
            if lookahead and bool(torch.isnan(first_stage[0]).any()):
                raise FloatingPointError("log_weight contains nan element(s)")
    except BaseException:
        inference._discard_pending_flags()
        raise
    if return_particles:
        particles = {"regimes": regimes, "means": means, "covariances": covariances, "log_weights": log_weights,
                     "ancestral_indices": ancestral, "indices": indices}
        if lookahead:
            particles["first_stage_log_weights"] = first_stage
        return path, particles
    return path


def switching_particle_gibbs(observations, model, num_particles, num_sweeps, reference=None, ancestor_sampling=True,
                             burn_in=0, observed=None, lookahead=False):
    """Runs `num_sweeps` sweeps of `conditional_switching_filter`, each from the path the one before returned: batch_size
    independent Markov chains on regime paths whose stationary law is p(s_{0:T-1} | y_{0:T-1}) for any num_particles; with
    ancestor sampling 8 .. 64 particles mix.

    reference: the first path, T int32 [batch_size] tensors; None — one trajectory of `switching_smooth` with num_particles
        particles (which consumes numpy's RandomState as `switching_filter` does; the sweeps draw from torch's generator).
    burn_in: the first `burn_in` sweeps are run and not returned.
    lookahead: `conditional_switching_filter`'s, for every sweep; with reference=None the first path then comes from
        `switching_smooth(..., lookahead=True)`.  False is today's chain, call for call.
    The other arguments, `observed` among them, are `conditional_switching_filter`'s.

    Returns a dict: regimes (T int32 [batch_size, num_sweeps - burn_in]: regimes[t][b, s] is s_t of chain b after sweep
    burn_in + s — the shape `switching_state_smooth` and `conditional_kalman_filter` take, successive sweeps of a chain being
    dependent draws) and smoothed_regime_probabilities ([T, batch_size, M] float64: the frequencies over the kept sweeps)."""
    num_sweeps, burn_in = int(num_sweeps), int(burn_in)
    if not 0 <= burn_in < num_sweeps:
        raise ValueError("switching_particle_gibbs: 0 <= burn_in < num_sweeps, got burn_in = {} and num_sweeps = {}".format(
            burn_in, num_sweeps))
    if reference is None:
        drawn, _ = switching_smooth(observations, model, num_particles, num_trajectories=1, observed=observed,
                                    **({"lookahead": True} if lookahead else {}))
        reference = [regime[:, 0].contiguous() for regime in drawn["regimes"]]
    path, kept = list(reference), []
    more = {"lookahead": True} if lookahead else {}
    for sweep in range(num_sweeps):
        path = conditional_switching_filter(observations, model, num_particles, path, ancestor_sampling=ancestor_sampling,
                                            observed=observed, **more)
        if sweep >= burn_in:
            kept.append(path)
    M = model.num_regimes
    regimes = [torch.stack([paths[time] for paths in kept], dim=1) for time in range(len(path))]
    with torch.no_grad():
        probabilities = torch.stack([
            torch.nn.functional.one_hot(regime.to(torch.int64).clamp(0, M - 1), M).to(torch.float64).mean(dim=1)
            for regime in regimes])
    return {"regimes": regimes, "smoothed_regime_probabilities": probabilities}


def switching_forecast(filtered, model, horizon, regime_uniforms=None):
    """What comes next: the predictive distributions of steps T .. T + horizon - 1 from the last stored system of one run of
    `switching_filter` or `adapted_switching_filter`.  A forecast step is the filter's step with nothing observed (K39 under
    an all-False mask, the identity ancestor): every particle draws its next regime from the transition's row and takes
    the Kalman prediction; its log-weight is 0, so the weights do not change and nothing is resampled.

    filtered: the dict either filter returned (the last of regimes, means, covariances; with `log_weights` the system is
        weighted by the last of them, without that key equally).
    horizon: H >= 1.
    regime_uniforms: None — torch.rand((batch_size, num_particles), float64) per step on the device; or a length-H sequence
        of such tensors (replay).

    Returns a dict: regimes (H int32 [batch_size, K]), means (H float64 [batch_size, K, D]), covariances (H float64
    [batch_size, K, D(D+1)/2], packed) — the predicted particle systems; log_weight [batch_size, K] (the filter's last,
    unchanged: zeros for an equally weighted system); regime_probabilities [H, batch_size, M], state_mean [H, batch_size, D],
    state_covariance [H, batch_size, D, D] (`switching_filter`'s three moments of those systems); observation_mean [H,
    batch_size, Dy] and observation_covariance [H, batch_size, Dy, Dy]: the moments of the mixture of N(C_s m + d_s, C_s P
    C_s^T + diag(r_s^2)) over the particles (plain torch per particle, the weighted means by K7).

    ValueError for an invalid model, a `filtered` without stored systems, horizon < 1 and regime_uniforms of the wrong length
    or shape; refusals and flags as `switching_filter`'s, read once at the end.  No host synchronisation inside the loop.
    Runs under torch.no_grad(): NOT differentiable."""
    name = "switching_forecast"
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("{}: horizon must be at least 1, got {}".format(name, horizon))
    if regime_uniforms is not None and len(regime_uniforms) != horizon:
        raise ValueError("{}: regime_uniforms must hold one tensor per forecast step ({}), got {}".format(
            name, horizon, len(regime_uniforms)))
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            ops = model.operands()
            M, D, Dy = model.num_regimes, model.latent_dim, model.observation_dim
            stored = filtered.get("regimes") if isinstance(filtered, dict) else None
            if not stored or not torch.is_tensor(stored[-1]) or stored[-1].dim() != 2:
                raise ValueError("{}: filtered must be the dict of switching_filter or adapted_switching_filter".format(name))
            batch_size, device = stored[-1].size(0), stored[-1].device
            regimes, means, covariances, log_weights, num_particles = _stored_systems(
                name, filtered, len(stored), batch_size, D, device)
            log_weight = log_weights[-1] if log_weights is not None else \
                torch.zeros((batch_size, num_particles), dtype=torch.float64, device=device)
            nothing = torch.zeros((batch_size, Dy), dtype=torch.float64, device=device)      # (never read into a chain)
            unobserved = torch.zeros((batch_size, Dy), dtype=torch.bool, device=device)
            _check_observations(name, provider, [nothing], model, num_particles)
            draw = _regime_draws(name, regime_uniforms, (batch_size, num_particles), device)
            state = (regimes[-1], means[-1], covariances[-1])
            out_regimes, out_means, out_covs = [], [], []
            for step in range(horizon):
                regime, mean, cov, _ = provider.switching_kalman_step(ops, state, None, draw(step), nothing,
                                                                      observed=unobserved)
                state = (regime, mean, cov)
                out_regimes.append(regime), out_means.append(mean), out_covs.append(cov)
            weights = [log_weight] * horizon
            state_mean, state_cov, probabilities = _moments(out_regimes, out_means, out_covs, weights, M)
            observation_mean, observation_cov = [], []
            for regime, mean, cov in zip(out_regimes, out_means, out_covs):
                s = regime.to(torch.int64).clamp(0, M - 1)
                C = ops["C"][s]                                                            # [B,K,Dy,D]
                center = torch.einsum("bkil,bkl->bki", C, mean) + ops["d"][s]
                spread = C @ unpack_covariance(cov, D) @ C.transpose(-1, -2) + torch.diag_embed(ops["r"][s] ** 2)
                second = spread + center.unsqueeze(-1) * center.unsqueeze(-2)
                average = statistics.empirical_mean(center, log_weight)
                second = statistics.empirical_mean(second.reshape(batch_size, num_particles, Dy * Dy),
                                                   log_weight).reshape(-1, Dy, Dy)
                observation_mean.append(average)
                observation_cov.append(second - average.unsqueeze(-1) * average.unsqueeze(-2))
            out = {"regimes": out_regimes, "means": out_means, "covariances": out_covs, "log_weight": log_weight,
                   "regime_probabilities": probabilities, "state_mean": state_mean, "state_covariance": state_cov,
                   "observation_mean": torch.stack(observation_mean),
                   "observation_covariance": torch.stack(observation_cov)}
            inference._raise_for_flags(provider.read_flags(device))
    except BaseException:
        inference._discard_pending_flags()
        raise
    return out


class _ZeroFeed:
    """A resampling feed that consumes no random numbers (`kalman_log_likelihood`: nothing is sampled)."""

    def __init__(self, block):
        self.block = block

    def next(self):
        return self.block


def kalman_log_likelihood(observations, model, observed=None):
    """The exact Kalman filter of a one-regime model on the device: `switching_filter` with M = 1 and one particle, where
    nothing is sampled.  Returns (log p(y_0..y_{T-1}) [batch_size] float64, filtered means [T,batch_size,D], filtered
    covariances [T,batch_size,D,D]).  observed: `switching_filter`'s — the Kalman filter with missing observations, still
    exact.  ValueError if the model has more than one regime."""
    if model.num_regimes != 1:
        raise ValueError("kalman_log_likelihood: the model has {} regimes; the Kalman filter is the one-regime case".format(
            model.num_regimes))
    if len(observations) == 0:
        raise ValueError("kalman_log_likelihood: observations must hold at least one timestep")
    shape = (observations[0].size(0), 1)
    zeros = [torch.zeros(shape, dtype=torch.float64, device=observations[0].device)] * len(observations)
    with inference.uniform_feed(_ZeroFeed(zeros[0][:, 0])):      # one particle: its own ancestor whatever the uniform
        out = switching_filter(observations, model, 1, resampling="systematic", regime_uniforms=zeros, observed=observed)
    D = model.latent_dim
    return (out["log_marginal_likelihood"], torch.stack([m[:, 0] for m in out["means"]]),
            torch.stack([unpack_covariance(c[:, 0], D) for c in out["covariances"]]))


# ---- EM: the expected sufficient statistics (K45 / K46), the M-step and the score -----------------------------------------------

PARAMETERS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
_STATISTICS = ("transition_counts", "next_next", "next_prev", "prev_prev", "obs_obs", "obs_state", "state_state",
               "initial_counts", "initial_state")


def _statistics_layout(D, Dy, masked):
    """name -> slice of the columns of K45 / K46's [16, F] array (include/aesmc_hip.h; `testing.switching_statistics.layout`)."""
    X = D + 1
    TX = X * (X + 1) // 2
    sizes = [("gram", TX), ("obs_obs", Dy), ("obs_state", Dy * X)] + ([("grams", Dy * TX)] if masked else []) + \
        [("counts", 16), ("next_next", D * (D + 1) // 2), ("next_prev", D * X), ("prev_prev", TX)]
    out, at = {}, 0
    for name, size in sizes:
        out[name] = slice(at, at + size)
        at += size
    return out


def _name_statistics(initial, later, M, D, Dy, masked):
    """The named statistics from the two [16, F] blocks (the t = 0 step's, the later steps')."""
    X = D + 1
    where = _statistics_layout(D, Dy, masked)
    total = initial + later
    gram = unpack_covariance(total[:M, where["gram"]], X)
    if masked:
        grams = unpack_covariance(total[:M, where["grams"]].reshape(M, Dy, X * (X + 1) // 2), X)
    else:
        grams = gram.unsqueeze(1).expand(M, Dy, X, X)
    first = unpack_covariance(initial[:M, where["gram"]], X)
    return {"transition_counts": later[:M, where["counts"]][:, :M].t().contiguous(),
            "next_next": unpack_covariance(later[:M, where["next_next"]], D),
            "next_prev": later[:M, where["next_prev"]].reshape(M, D, X),
            "prev_prev": unpack_covariance(later[:M, where["prev_prev"]], X),
            "obs_obs": total[:M, where["obs_obs"]],
            "obs_state": total[:M, where["obs_state"]].reshape(M, Dy, X),
            "state_state": grams,
            "initial_counts": first[:, D, D].clone(),
            "initial_state": first.sum(dim=0)}


def _check_smoothed(name, smoothed, observations, device):
    """(B, N, D, Dy) of the per-trajectory moments of a state smoother, or ValueError."""
    keys = ("regimes", "means", "covariances", "cross_covariances")
    if not isinstance(smoothed, dict) or any(key not in smoothed for key in keys):
        raise ValueError("{}: smoothed must be a dict with {} (switching_state_smooth(..., return_trajectories=True))".format(
            name, ", ".join(keys)))
    num_timesteps = len(observations)
    for key in keys:
        wanted = num_timesteps - 1 if key == "cross_covariances" else num_timesteps
        if len(smoothed[key]) != wanted:
            raise ValueError("{}: smoothed[{!r}] must hold {} tensors, got {}".format(name, key, wanted, len(smoothed[key])))
    first = smoothed["means"][0]
    if not torch.is_tensor(first) or first.dim() != 3:
        raise ValueError("{}: smoothed['means'][0] must be a [batch_size, num_trajectories, D] float64 tensor".format(name))
    B, N, D = first.shape
    for y in observations:
        if not torch.is_tensor(y) or y.dim() != 2 or tuple(y.shape) != tuple(observations[0].shape) or \
                y.dtype not in (torch.float32, torch.float64) or y.device != device:
            raise ValueError("{}: observations must be [batch_size, Dy] float32 or float64 tensors on one device".format(name))
    if observations[0].size(0) != B:
        raise ValueError("{}: the observations have {} batch rows, the moments {}".format(name, observations[0].size(0), B))
    shapes = {"regimes": ((B, N), torch.int32), "means": ((B, N, D), torch.float64),
              "covariances": ((B, N, D * (D + 1) // 2), torch.float64), "cross_covariances": ((B, N, D, D), torch.float64)}
    for key in keys:
        shape, dtype = shapes[key]
        for time, tensor in enumerate(smoothed[key]):
            if not torch.is_tensor(tensor) or tuple(tensor.shape) != shape or tensor.dtype != dtype or tensor.device != device:
                raise ValueError("{}: smoothed[{!r}][{}] must be {} {} on {}".format(name, key, time, shape, dtype, device))
    return B, N, D, observations[0].size(1)


def switching_expected_statistics(smoothed, observations, model_or_num_regimes, observed=None):
    """The E-step's reduction: the expected complete-data sufficient statistics of a `SwitchingLinearGaussian`, summed over
    time, batch rows and trajectories, from the per-trajectory smoothed moments — what `switching_m_step` and
    `switching_score` take.  With x = (z, 1), X = D + 1, j = s_t, i = s_{t-1} and o_c whether component c of y_t[b] was observed:

        transition_counts [M, M]  (as [i, j])   1[s_{t-1} = i]             next_next [M, D, D]   E[z_t z_t^T]
        next_prev [M, D, X]   E[z_t x_{t-1}^T]                             prev_prev [M, X, X]   E[x_{t-1} x_{t-1}^T]      (t >= 1)
        obs_obs [M, Dy]   o_c y_c^2        obs_state [M, Dy, X]   o_c y_c E[x_t]^T        state_state [M, Dy, X, X]   o_c E[x_t x_t^T]
        initial_counts [M]   1[s_0 = j]    initial_state [X, X]   E[x_0 x_0^T]

    smoothed: a dict with regimes (T int32 [batch_size, N]), means (T float64 [batch_size, N, D]), covariances (T packed) and
    cross_covariances (T-1 [batch_size, N, D, D]): what `switching_smooth_states(..., return_trajectories=True)` or
    `switching_state_smooth(..., return_trajectories=True)` (with the regimes it was given) returns.  observations, observed:
    as `switching_filter`'s.  model_or_num_regimes: the model, or M.

    One launch per timestep — K45 (`aesmc_switching_moment_statistics`), with a mask K46: one lane per trajectory forms its
    terms in float64 and the float64 matrix cores sum them per regime against the indicator of s_t, without atomics and in a
    fixed order (the same inputs give the same bits) — the t = 0 step into a block of its own, then one finishing launch per
    block.  Returns the float64 tensors above on the device (without a mask state_state is a stride-0 expansion of one gram)
    with batch_size, num_trajectories and num_timesteps.

    ValueError for operands that disagree and — read once, at the end, with the flags — a regime outside [0, M);
    FloatingPointError if a statistic is NaN (a NaN moment, or a NaN observation at an observed position);
    NotImplementedError naming the covered class past the limits.  No host synchronisation inside the loop; an exception on
    the way discards whatever was flagged.  N == 0 gives zeros without a launch; T == 1 launches only the t = 0 form."""
    name = "switching_expected_statistics"
    provider = _kernels.get()
    try:
        with torch.no_grad(), _syncfree.scope():
            num_timesteps = len(observations)
            if num_timesteps == 0:
                raise ValueError("{}: observations must hold at least one timestep".format(name))
            M = model_or_num_regimes.num_regimes if isinstance(model_or_num_regimes, SwitchingLinearGaussian) else \
                int(model_or_num_regimes)
            if M < 1:
                raise ValueError("{}: the number of regimes must be at least 1, got {}".format(name, M))
            device = observations[0].device if torch.is_tensor(observations[0]) else None
            B, N, D, Dy = _check_smoothed(name, smoothed, observations, device)
            if isinstance(model_or_num_regimes, SwitchingLinearGaussian) and \
                    (model_or_num_regimes.latent_dim, model_or_num_regimes.observation_dim) != (D, Dy):
                raise ValueError("{}: the model has D = {} and Dy = {}, the moments and observations {} and {}".format(
                    name, model_or_num_regimes.latent_dim, model_or_num_regimes.observation_dim, D, Dy))
            mask = _observed_steps(name, observed, observations)
            if M > MAX_REGIMES:
                _refuse("a model of {} regimes (M > {})".format(M, MAX_REGIMES))
            if not 1 <= D <= MAX_LATENT_DIM:
                _refuse("a latent of {} values (D > {})".format(D, MAX_LATENT_DIM))
            if not 1 <= Dy <= MAX_OBSERVATION_DIM:
                _refuse("an observation of {} values (Dy > {})".format(Dy, MAX_OBSERVATION_DIM))
            if B * N > 0x7fffffff // (MAX_LATENT_DIM * MAX_LATENT_DIM):
                _refuse("{} trajectories in {} batch rows (batch_size * num_trajectories * D^2 beyond 32-bit element arithmetic)"
                        .format(N, B))
            if provider.name == "hip":
                _kernels._require_hip(observations[0], "observations")      # (no CPU fallback)
            masks = [mask(time) for time in range(num_timesteps)]
            masked = any(masks)
            sizes = dict(batch_size=B, num_trajectories=N, num_timesteps=num_timesteps)
            if N == 0 or B == 0:
                zeros = torch.zeros((16, provider.switching_statistics_columns(D, Dy, masked)), dtype=torch.float64, device=device)
                return dict(_name_statistics(zeros, zeros, M, D, Dy, masked), **sizes)
            everything = torch.ones((B, Dy), dtype=torch.bool, device=device) if masked else None
            regimes, means, covs, crosses = (smoothed[key] for key in ("regimes", "means", "covariances", "cross_covariances"))
            for time in range(num_timesteps):
                seen = {"observed": masks[time].get("observed", everything)} if masked else {}
                previous = None if time == 0 else (regimes[time - 1], means[time - 1], covs[time - 1], crosses[time - 1])
                provider.switching_statistics_step(observations[time], regimes[time], means[time], covs[time], M,
                                                   previous=previous, block=min(time, 1), accumulate=time > 1, **seen)
            initial = provider.switching_statistics_finish(observations[0], B, N, D, Dy, masked, block=0)
            later = provider.switching_statistics_finish(observations[0], B, N, D, Dy, masked, block=1) \
                if num_timesteps > 1 else torch.zeros_like(initial)
            out = _name_statistics(initial, later, M, D, Dy, masked)
            flags = provider.read_flags(device)
            if flags & _lib.FLAG_INDEX_OUT_OF_RANGE:      # (the kernels raise it themselves: no pass over the regimes here)
                raise ValueError("{}: regimes holds a value outside [0, M)".format(name))
            inference._raise_for_flags(flags)
            if bool((torch.isnan(initial).any() | torch.isnan(later).any())):
                raise FloatingPointError("a statistic contains nan element(s)")
    except BaseException:
        inference._discard_pending_flags()
        raise
    return dict(out, **sizes)


def _check_statistics(name, statistics, model):
    if not isinstance(model, SwitchingLinearGaussian):
        raise ValueError("{}: the model must be a SwitchingLinearGaussian, got {}".format(name, type(model).__name__))
    keys = _STATISTICS + ("batch_size", "num_trajectories", "num_timesteps")
    if not isinstance(statistics, dict) or any(key not in statistics for key in keys):
        raise ValueError("{}: statistics must be what switching_expected_statistics returns".format(name))
    M, D, Dy = model.num_regimes, model.latent_dim, model.observation_dim
    if tuple(statistics["next_prev"].shape) != (M, D, D + 1) or tuple(statistics["obs_state"].shape) != (M, Dy, D + 1):
        raise ValueError("{}: the statistics are those of M = {}, D = {}, Dy = {}; the model has {}, {}, {}".format(
            name, statistics["next_prev"].size(0), statistics["next_prev"].size(1), statistics["obs_state"].size(1), M, D, Dy))
    device = statistics["next_prev"].device
    if model.pi0.device != device:
        raise ValueError("{}: the model is on {}, the statistics on {}".format(name, model.pi0.device, device))
    for key, shape in (("A", (D, D)), ("b", (D,)), ("q", (D,)), ("C", (Dy, D)), ("d", (Dy,)), ("r", (Dy,))):
        value = getattr(model, key)
        if value.dim() != len(shape) + 1 or value.size(0) not in (1, M) or tuple(value.shape[1:]) != shape:
            raise ValueError("{}: {} must be {} (or a leading 1: shared across regimes), got {}".format(
                name, key, (M,) + shape, tuple(value.shape)))
    if tuple(model.m0.shape) != (D,) or model.s0.numel() not in (1, D):
        raise ValueError("{}: m0 must be [{}] and s0 hold one value or {}".format(name, D, D))
    return M, D, Dy


def _quadratic(square, cross, gram, weights):
    """square - 2 w . cross + w gram w^T for every row w of weights [M, R, X] (gram [M, R, X, X])."""
    return square - 2.0 * (weights * cross).sum(dim=-1) + torch.einsum("mri,mril,mrl->mr", weights, gram, weights)


def _affine_block(statistics, D, emission):
    """(square [M,R], cross [M,R,X], gram [M,R,X,X], count [M,R]) of the transition's or the emission's regression."""
    if emission:
        grams = statistics["state_state"]
        return statistics["obs_obs"], statistics["obs_state"], grams, grams[:, :, D, D]
    lagged = statistics["prev_prev"]
    M, X = lagged.size(0), D + 1
    return (torch.diagonal(statistics["next_next"], dim1=-2, dim2=-1), statistics["next_prev"],
            lagged.unsqueeze(1).expand(M, D, X, X), lagged[:, D, D].unsqueeze(1).expand(M, D))


def _affine_update(previous, names, block, learn):
    """The new (weights, offsets, scales) of one affine-Gaussian block, `testing.switching_statistics._affine_update`."""
    prev_w, prev_b, prev_scale = (getattr(previous, key) for key in names)
    learn_w, learn_b, learn_scale = (key in learn for key in names)
    square, cross, gram, count = block
    M, R, X = cross.shape
    if prev_w.size(0) != prev_b.size(0):
        raise NotImplementedError("switching_m_step: {} and {} must both be shared across regimes or neither".format(*names[:2]))
    pool = lambda value, shared: value.sum(dim=0, keepdim=True) if shared else value
    w_shared, s_shared = prev_w.size(0) == 1 and M > 1, prev_scale.size(0) == 1 and M > 1
    weights = torch.cat([prev_w, prev_b.unsqueeze(-1)], dim=-1)
    if learn_w or learn_b:
        device = cross.device
        free = torch.tensor([i for i in range(X) if (learn_w if i < X - 1 else learn_b)], dtype=torch.int64, device=device)
        fixed = torch.tensor([i for i in range(X) if not (learn_w if i < X - 1 else learn_b)], dtype=torch.int64, device=device)
        pooled_gram, pooled_cross = pool(gram, w_shared), pool(cross, w_shared)
        held = weights.index_select(-1, fixed).unsqueeze(-2)                                          # [., R, 1, fixed]
        target = pooled_cross.index_select(-1, free).unsqueeze(-2) - \
            held @ pooled_gram.index_select(-2, fixed).index_select(-1, free)
        solved = target @ torch.linalg.pinv(pooled_gram.index_select(-2, free).index_select(-1, free), hermitian=True)
        estimate = weights.clone()
        estimate[..., free] = solved.squeeze(-2)
        weights = torch.where((pool(count, w_shared) > 0).unsqueeze(-1), estimate, weights)
    scale = prev_scale
    if learn_scale:
        quad = pool(_quadratic(square, cross, gram, weights.expand(M, R, X)), s_shared)
        total = pool(count, s_shared)
        estimate = torch.sqrt(quad.clamp_min(0.0) / total.clamp_min(1e-300))
        scale = torch.where(total > 0, estimate, prev_scale)
    return weights[..., :-1].contiguous(), weights[..., -1].contiguous(), scale


def switching_m_step(statistics, previous, learn=PARAMETERS):
    """The closed-form M-step of EM for a `SwitchingLinearGaussian`: a NEW model that maximises the expected complete-data
    log-likelihood `statistics` (`switching_expected_statistics`'s) stands for, in the parameters named by `learn` (a tuple
    of names out of PARAMETERS; default: all ten); every other buffer is copied from `previous`.  Plain torch float64 on the
    statistics' device — the matrices are tiny.

        pi0 = initial_counts / (batch_size N)            Pi[i, :] = transition_counts[i, :] / its sum
        m0, s0 from initial_state                        [A_j b_j] = next_prev[j] pinv(prev_prev[j])     (hermitian pinv)
        q_ji^2 = (next_next_ii - 2 w . next_prev_i + w prev_prev w^T) / n_j,  w = [A_j b_j]_i, clamped at 0
        row c of [C_j d_j], r_jc: the same regression on obs_state, state_state[:, c] and obs_obs

    A row of Pi with no departures, a regime never visited and a component never observed under a regime keep `previous`'s
    values.  With only one of A, b (C, d) learned the other is held in the regression.  A parameter `previous` holds with a
    leading extent of 1 (shared across regimes) is estimated from the statistics summed over the regimes and keeps that
    shape; A with b (C with d) must then both be shared or neither (NotImplementedError).  The contract is
    `aesmc_amd.testing.switching_statistics.m_step`."""
    name = "switching_m_step"
    M, D, Dy = _check_statistics(name, statistics, previous)
    learn = tuple(learn)
    unknown = sorted(set(learn) - set(PARAMETERS))
    if unknown:
        raise ValueError("{}: learn names {}; the parameters are {}".format(name, unknown, PARAMETERS))
    with torch.no_grad():
        new = {key: getattr(previous, key).clone() for key in PARAMETERS}
        if "pi0" in learn:
            new["pi0"] = statistics["initial_counts"] / float(statistics["batch_size"] * statistics["num_trajectories"])
        if "Pi" in learn:
            departures = statistics["transition_counts"].sum(dim=1, keepdim=True)
            new["Pi"] = torch.where(departures > 0, statistics["transition_counts"] / departures.clamp_min(1.0), new["Pi"])
        first = statistics["initial_state"]
        total, seen = first[D, D].clamp_min(1e-300), first[D, D] > 0
        if "m0" in learn:
            new["m0"] = torch.where(seen, first[:D, D] / total, new["m0"])
        if "s0" in learn:
            m0 = new["m0"]
            quad = (torch.diagonal(first)[:D] - 2.0 * m0 * first[:D, D] + m0 * m0 * first[D, D]).clamp_min(0.0)
            estimate = torch.sqrt(quad / total) if previous.s0.numel() == D else torch.sqrt(quad.sum() / (D * total)).reshape(1)
            new["s0"] = torch.where(seen, estimate.reshape(previous.s0.shape), new["s0"])
        new["A"], new["b"], new["q"] = _affine_update(previous, ("A", "b", "q"), _affine_block(statistics, D, False), learn)
        new["C"], new["d"], new["r"] = _affine_update(previous, ("C", "d", "r"), _affine_block(statistics, D, True), learn)
        return SwitchingLinearGaussian(**new)


def switching_score(statistics, model):
    """The score by Fisher's identity: a dict with the gradient, with respect to each buffer of `model` in the buffer's own
    shape, of the Monte Carlo estimate of sum_b log p(y^b) — (1/N) sum_{b,n} E[grad log p(y^b, z, s^{b,n}) | y^b, s^{b,n}], from
    `switching_expected_statistics`'s sums alone: no adjoint of the filters' Cholesky chains is needed.  For [A b]:
    diag(q_j^-2) (next_prev[j] - [A_j b_j] prev_prev[j]) / N; for q: (-n_j / q + quadratic / q^3) / N; likewise C, d, r, m0 and
    s0; for Pi and pi0 the plain partial derivatives count / probability (0 where the count is 0; the simplex is the caller's
    business).  A shared parameter (leading extent 1) receives the sum over the regimes.  The trajectories must be (as
    `switching_smooth_states` draws them) samples of p(s | y) under `model` for the estimate to be the score at `model`.  The
    contract is `aesmc_amd.testing.switching_statistics.score`."""
    M, D, Dy = _check_statistics("switching_score", statistics, model)
    N = float(statistics["num_trajectories"])
    out = {}
    with torch.no_grad():
        for names, emission in ((("A", "b", "q"), False), (("C", "d", "r"), True)):
            w, b, scale = (getattr(model, key) for key in names)
            square, cross, gram, count = _affine_block(statistics, D, emission)
            R, X = cross.size(1), D + 1
            weights = torch.cat([w.expand((M,) + tuple(w.shape[1:])), b.expand((M,) + tuple(b.shape[1:])).unsqueeze(-1)], dim=-1)
            sigma = scale.expand(M, R)
            residual = (cross - torch.einsum("mrl,mrlk->mrk", weights, gram)) / (sigma * sigma).unsqueeze(-1) / N
            grad_scale = (-count / sigma + _quadratic(square, cross, gram, weights) / sigma ** 3) / N
            fold = lambda grad, like: grad.sum(dim=0, keepdim=True) if like.size(0) == 1 and M > 1 else grad
            out[names[0]], out[names[1]], out[names[2]] = \
                fold(residual[..., :-1], w), fold(residual[..., -1], b), fold(grad_scale, scale)
        first = statistics["initial_state"]
        m0, s0 = model.m0, model.s0.reshape(-1).expand(D)
        out["m0"] = (first[:D, D] - m0 * first[D, D]) / (s0 * s0) / N
        quad = torch.diagonal(first)[:D] - 2.0 * m0 * first[:D, D] + m0 * m0 * first[D, D]
        grad_s0 = (-first[D, D] / s0 + quad / s0 ** 3) / N
        out["s0"] = (grad_s0 if model.s0.numel() == D else grad_s0.sum().reshape(1)).reshape(model.s0.shape)
        counts, starts = statistics["transition_counts"], statistics["initial_counts"]
        out["Pi"] = torch.where(counts > 0, counts / model.Pi, torch.zeros_like(counts)) / N
        out["pi0"] = torch.where(starts > 0, starts / model.pi0, torch.zeros_like(starts)) / N
    return out
