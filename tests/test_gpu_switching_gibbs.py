"""Particle Gibbs on the regimes of a switching linear-Gaussian model on the device: kernel K37
(aesmc_switching_conditional_ancestor_index) against its NumPy contract (aesmc_amd/testing/rao_blackwell.py) index for index
and against the launches it replaces, its bad rows, the entry K38 (aesmc_switching_kalman_conditional_step) against K31 bit for
bit, the C ABI's refusals, and `aesmc_amd.rao_blackwell.conditional_switching_filter` / `switching_particle_gibbs` end to end:
replayed against the contract's pass, their properties, and the invariance and mixing of the chain against the enumeration of
all regime sequences."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from tests.test_switching_gibbs_contract import (CHAINS, assert_within_five_standard_errors, invariance_case, resampling_case,
                                                 sweep_case)

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("pi0", "Pi", "m0", "s0", "A", "b", "q", "C", "d", "r")
# (B, K, M, D, Dy): one lane; two particles (one free slot); a partial wavefront; 65 particles (the first size on 256 lanes)
# with the covariances in LDS; several particles per lane; the largest M; a row of four particles per lane; and the particle
# cap of each padded extent of D (2, 4, 8)
SHAPES = [(1, 1, 1, 1, 1), (3, 2, 2, 2, 1), (3, 7, 2, 2, 1), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3), (1, 257, 16, 8, 1),
          (2, 1025, 2, 3, 2), (1, 8192, 2, 2, 1), (1, 8192, 2, 4, 2), (1, 4096, 2, 8, 2)]


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device):
    return None if array is None else torch.from_numpy(np.array(array)).to(device)


def _torch_model(ops, device):
    from aesmc_amd import rao_blackwell
    return rao_blackwell.SwitchingLinearGaussian(*[torch.from_numpy(ops[name].copy()) for name in MODEL_KEYS]).to(device)


def _device_index(provider, device, log_w, u, log_Pi, regime_next, F, lam, particles):
    return provider.switching_conditional_ancestor_index(
        _dev(log_w, device), _dev(u, device), _dev(log_Pi, device), _dev(regime_next, device), _dev(F, device),
        _dev(lam, device), tuple(_dev(part, device) for part in particles))


@pytest.mark.parametrize("steps", [1, 2, 3])      # the first (NULL) step; a rank-deficient Om handed over where Dy < D; a later one
@pytest.mark.parametrize("B,K,M,D,Dy", SHAPES)
def test_the_ancestors_equal_the_contract_and_the_launches_they_replace(hip_device, B, K, M, D, Dy, steps):
    """First, from the contract alone (a property of the seeds): no pinned draw lies within 4 times its scores' bound of a
    step of the running sum — a score off by e moves a normalised partial sum by at most exp(2 e) - 1 <= 4 e — nor within
    what K float64 weights, each exp to two units in the last place, can move it (8 K u), and no free draw within the
    latter.  Then every index is equal; no share is excused.  Then, on the device: the pinned column is K21's draw from
    K35's scores with N = 1 at the same uniform, the free columns are K26's."""
    provider = _provider()
    model, log_Pi, regime_next, F, lam, particles, log_w, u = resampling_case(B, K, M, D, Dy, steps)
    want, flags, margins, bound = contract.switching_conditional_ancestor_index(log_w, u, log_Pi, regime_next, F, lam, particles)
    rounding = 8 * K * contract.UNIT
    assert flags == 0
    if K > 1:
        print("smallest free margin", margins[:, :K - 1].min(), "smallest pinned margin", margins[:, K - 1].min(),
              "largest score bound", bound.max())
        assert (margins[:, :K - 1] > rounding).all()
        assert (margins[:, K - 1] > 4.0 * bound + rounding).all()
    got = _device_index(provider, hip_device, log_w, u, log_Pi, regime_next, F, lam, particles)
    assert provider.read_flags(hip_device) == 0 and got.dtype == torch.int64 and got.shape == (B, K)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    plain = _device_index(provider, hip_device, log_w, u, log_Pi, regime_next, None, None, particles)
    assert provider.read_flags(hip_device) == 0
    assert torch.equal(plain[:, :K - 1], got[:, :K - 1]) and bool((plain[:, K - 1] == K - 1).all())
    # the composition: K35 with N = 1, K21 on its scores, K26 without a transition term
    state = tuple(_dev(part, hip_device) for part in particles)
    scores = provider.switching_backward_scores(_dev(log_Pi, hip_device), _dev(regime_next[:, None], hip_device),
                                                _dev(F[:, None, :], hip_device), _dev(lam[:, None, :], hip_device), state,
                                                _dev(log_w, hip_device))
    pinned, _ = provider.backward_sample(scores[:, 0, :], None, None, None, _dev(u[:, K - 1:], hip_device))
    free = provider.conditional_ancestor_index(_dev(log_w, hip_device), _dev(u, hip_device))
    assert provider.read_flags(hip_device) == 0
    assert torch.equal(got[:, K - 1], pinned[:, 0]) and torch.equal(got[:, :K - 1], free[:, :K - 1])


def test_bad_rows_leave_every_other_row_as_it_was(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 5, 300, 4, 5, 3
    model, log_Pi, regime_next, F, lam, particles, log_w, u = resampling_case(B, K, M, D, Dy, 2)
    run = lambda **kw: _device_index(provider, hip_device, kw.get("log_w", log_w), u, kw.get("log_Pi", log_Pi),
                                     kw.get("regime_next", regime_next), F, lam, kw.get("particles", particles)).cpu().numpy()
    clean = run()
    assert provider.read_flags(hip_device) == 0
    # a NaN weight: every slot of the row
    poisoned = log_w.copy()
    poisoned[1, 77] = np.nan
    got = run(log_w=poisoned)
    assert provider.read_flags(hip_device) == contract.FLAG_NAN_LOG_WEIGHT
    assert (got[1] == K).all() and np.array_equal(np.delete(got, 1, 0), np.delete(clean, 1, 0))
    # every transition into s' impossible: the pinned slot of the rows that enter it
    blocked = log_Pi.copy()
    blocked[:, regime_next[0]] = -np.inf
    hit = regime_next == regime_next[0]
    got = run(log_Pi=blocked)
    assert provider.read_flags(hip_device) == contract.FLAG_DEGENERATE_ROW
    assert (got[hit, K - 1] == K).all() and np.array_equal(got[:, :K - 1], clean[:, :K - 1])
    assert np.array_equal(got[~hit, K - 1], clean[~hit, K - 1])
    # a NaN mean: the pinned slot of its row
    mean = particles[1].copy()
    mean[3, 299, 4] = np.nan
    got = run(particles=(particles[0], mean, particles[2]))
    assert provider.read_flags(hip_device) == contract.FLAG_NAN_LOG_WEIGHT
    assert got[3, K - 1] == K and np.array_equal(got[:, :K - 1], clean[:, :K - 1])
    assert np.array_equal(np.delete(got, 3, 0), np.delete(clean, 3, 0))
    # a regime outside [0, M) on either side
    regime = particles[0].copy()
    regime[0, 4], regime[4, 256] = M, -1
    got = run(particles=(regime, particles[1], particles[2]))
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT
    assert got[0, K - 1] == K and got[4, K - 1] == K and np.array_equal(got[:, :K - 1], clean[:, :K - 1])
    assert np.array_equal(got[1:4], clean[1:4])
    outside = regime_next.copy()
    outside[2] = M
    got = run(regime_next=outside)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT
    assert got[2, K - 1] == K and np.array_equal(got[:, :K - 1], clean[:, :K - 1])
    assert np.array_equal(np.delete(got, 2, 0), np.delete(clean, 2, 0))
    want, flags, _, _ = contract.switching_conditional_ancestor_index(log_w, u, log_Pi, outside, F, lam, particles)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("later,index", [(False, "none"), (True, "none"), (True, "unsorted")])
@pytest.mark.parametrize("B,K,M,D,Dy", contract.STEP_SHAPES)
def test_the_conditional_step_is_k31_bit_for_bit(hip_device, B, K, M, D, Dy, later, index):
    """Slots 0 .. K-2 equal K31 on the same inputs bitwise; slot K-1 equals K31 under the forced cumulative rows of
    `_conditional_filter` for the pinned regime bitwise: regime, mean, covariance and log-weight.  And K31 itself, through
    its own entry (no pinned regimes), is still its contract's: the regimes equal, the rest within the bounds."""
    provider = _provider()
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index=index, later=later)
    pinned = np.random.default_rng([B, K, M, 38]).integers(0, M, B).astype(np.int32)
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    dev_state = None if state is None else tuple(_dev(part, hip_device) for part in state)
    args = (dev_state, _dev(idx, hip_device), _dev(uniforms, hip_device))
    got = provider.switching_kalman_conditional_step(ops, *args, _dev(pinned, hip_device), _dev(y, hip_device))
    plain = provider.switching_kalman_step(ops, *args, _dev(y, hip_device))
    edges = (torch.arange(M, dtype=torch.float64, device=hip_device) + 1.0) / M
    forced = dict(ops, cdf0=edges, cdf=edges.expand(M, M).contiguous())
    forced_u = ((_dev(pinned, hip_device).to(torch.float64) + 0.5) / M).unsqueeze(1).expand(B, K).contiguous()
    pin = provider.switching_kalman_step(forced, dev_state, args[1], forced_u, _dev(y, hip_device))
    assert provider.read_flags(hip_device) == 0
    assert torch.equal(got[0][:, K - 1].cpu(), torch.from_numpy(pinned))
    for part, free, last in zip(got, plain, pin):
        assert torch.equal(part[:, :K - 1], free[:, :K - 1]) and torch.equal(part[:, K - 1], last[:, K - 1])
    want = contract.switching_kalman_step(model, state, idx, uniforms, y)
    bounds = contract.switching_kalman_step_bound(model, state, idx, uniforms, y)
    assert np.array_equal(plain[0].cpu().numpy(), want[0])
    for part, expected, bound in zip(plain[1:], want[1:4], bounds):
        assert (np.abs(part.cpu().numpy() - expected) <= bound).all()
    # a pinned regime outside [0, M): that slot alone, flagged as a stored regime outside it
    bad = pinned.copy()
    bad[B - 1] = M
    out = provider.switching_kalman_conditional_step(ops, *args, _dev(bad, hip_device), _dev(y, hip_device))
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    assert int(out[0][B - 1, K - 1]) == 0 and bool(torch.isnan(out[3][B - 1, K - 1]))
    assert bool(torch.isnan(out[1][B - 1, K - 1]).all()) and bool(torch.isnan(out[2][B - 1, K - 1]).all())
    keep = torch.ones((B, K), dtype=torch.bool, device=hip_device)
    keep[B - 1, K - 1] = False
    for part, reference in zip(out, got):
        assert torch.equal(part[keep], reference[keep])


@pytest.mark.parametrize("B,K,M,D,Dy", [(3, 7, 2, 2, 1), (2, 65, 3, 8, 8)])
def test_the_draw_entry_is_still_its_contracts(hip_device, B, K, M, D, Dy):
    """K33 through its own entry, which hands the kernel no pinned regimes: regimes equal, the rest within the bounds."""
    provider = _provider()
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index="unsorted")
    log_w, cdf, flags = contract.switching_lookahead(model, np.log(model["Pi"]), state, y)
    assert flags == 0
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    got = provider.switching_kalman_draw(ops, tuple(_dev(part, hip_device) for part in state), _dev(idx, hip_device),
                                         _dev(uniforms, hip_device), _dev(cdf, hip_device), _dev(y, hip_device))
    assert provider.read_flags(hip_device) == 0
    want = contract.switching_kalman_draw(model, state, idx, uniforms, cdf, y)
    bounds = contract.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y)
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    for part, expected, bound in zip(got[1:], want[1:4], bounds):
        assert (np.abs(part.cpu().numpy() - expected) <= bound).all()


def test_the_abi_refuses_bad_arguments_without_a_launch(hip_device):
    """Device pointers this time: a refusal must leave the outputs as they were."""
    from aesmc_amd import _lib
    lib = _lib.load()
    B, K, M, D, Dy = 2, 7, 2, 2, 1
    model, log_Pi, regime_next, F, lam, particles, log_w, u = resampling_case(B, K, M, D, Dy, 2)
    operands = [_dev(part, hip_device) for part in (log_w, u, log_Pi, regime_next, F, lam) + tuple(particles)]
    out = torch.full((B, K), 7, dtype=torch.int64, device=hip_device)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(operands=operands, out=out, B=B, K=K, M=M, D=D):
        return lib.aesmc_switching_conditional_ancestor_index(*[ptr(t) for t in operands], ptr(out), None, B, K, M, D, None)

    assert call(operands=[None] + operands[1:]) == 1 and call(out=None) == 1 and call(out=operands[0]) == 1
    assert call(operands=operands[:4] + [None] + operands[5:]) == 1                                 # factor without lambda
    assert call(operands=operands[:6] + [None] + operands[7:]) == 1                                 # no stored regimes
    assert call(K=-1) == 1 and call(M=0) == 1 and call(D=0) == 1
    assert call(D=9) == 2 and call(M=17) == 2 and call(K=8193) == 2 and call(K=4097, D=5) == 2
    assert call(B=0) == 0 and call(K=0) == 0
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    keys = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    block = lambda **kw: _lib.SwitchingModel(*([ops[name].data_ptr() for name in keys] + [kw.get("M", M), kw.get("D", D),
                                                                                          kw.get("Dy", Dy)]))
    state = operands[6:]
    idx = torch.zeros((B, K), dtype=torch.int64, device=hip_device)
    y = torch.zeros((B, Dy), dtype=torch.float64, device=hip_device)
    outs = [torch.full((B, K), 7, dtype=torch.int32, device=hip_device)] + \
        [torch.full(shape, 7.0, dtype=torch.float64, device=hip_device) for shape in ((B, K, D), (B, K, 3), (B, K))]

    def step(model=None, state=state, idx=idx, uniforms=operands[1], pinned=operands[3], y=y, outs=outs, B=B, K=K, dtype=1):
        model = block() if model is None else model
        return lib.aesmc_switching_kalman_conditional_step(dtype, ctypes.byref(model), *[ptr(t) for t in state], ptr(idx),
                                                           ptr(uniforms), ptr(pinned), ptr(y), *[ptr(t) for t in outs], None,
                                                           B, K, None)

    assert step(pinned=None) == 1 and step(uniforms=None) == 1 and step(y=None) == 1 and step(dtype=5) == 1
    assert step(state=[None] + state[1:]) == 1 and step(outs=outs[:3] + [None]) == 1 and step(outs=[state[0]] + outs[1:]) == 1
    assert step(pinned=outs[0]) == 1 and step(B=-1) == 1
    assert step(model=block(D=9)) == 2 and step(model=block(M=17)) == 2 and step(B=1 << 16, K=1 << 16) == 2
    assert step(B=0) == 0 and step(K=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and all(bool((t == 7).all()) for t in outs)


@pytest.mark.parametrize("ancestor_sampling", [True, False])
@pytest.mark.parametrize("B,K,M,D,Dy,seed", [(2, 300, 4, 5, 3, 0), (3, 65, 3, 8, 8, 0)])
def test_a_whole_sweep_on_replayed_uniforms_equals_the_contracts_pass(hip_device, B, K, M, D, Dy, seed, ancestor_sampling):
    """The rule of `test_backward_simulation_on_replayed_uniforms_equals_the_contracts_pass`: every index and regime is equal,
    except in rows where a draw's contract margin is within what scores (or log-weights) off by their bounds can move the
    normalised running sum, 4 e with e the pinned scores' bound, the propagated tolerance of the log-weights and the
    rounding of K weights summed; a row excused once is excused from there on (it walks another path).  The excused draws may
    be at most 0.1 % of all; with float64 scores the expected number is zero.  Means, covariances and log-weights of the
    rows never excused lie within the contract's propagated tolerances."""
    from aesmc_amd import rao_blackwell
    T = 5
    ops, _, _, reference, uniforms, regime_u = sweep_case(T, B, K, M, D, Dy, seed)
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=seed + 1)
    dev = lambda blocks: [_dev(block, hip_device) for block in blocks]
    path, particles = rao_blackwell.conditional_switching_filter(
        observations, model, K, dev(reference), ancestor_sampling=ancestor_sampling, uniforms=dev(uniforms),
        regime_uniforms=dev(regime_u), return_particles=True)
    want = contract.conditional_switching_pass([y.cpu().numpy() for y in observations], ops, K, reference, uniforms, regime_u,
                                               ancestor_sampling=ancestor_sampling)
    assert want["flags"] == 0
    rounding = 8 * K * contract.UNIT
    excused = np.zeros(B, dtype=bool)
    count = 0
    for t in range(T):
        if t > 0:
            carried = want["tolerances"]["log_weights"][t - 1] + rounding
            margins = want["margins"][t - 1]
            near = (margins[:, :K - 1] <= 4.0 * carried).any(axis=1) | \
                (margins[:, K - 1] <= 4.0 * (carried + want["score_bounds"][t - 1]))
            count += int((margins[:, :K - 1] <= 4.0 * carried).sum() +
                         (margins[:, K - 1] <= 4.0 * (carried + want["score_bounds"][t - 1])).sum())
            excused |= near
            index = particles["ancestral_indices"][t - 1].cpu().numpy()
            differs = (index != want["ancestral_indices"][t - 1]).any(axis=1)
            assert not (differs & ~excused).any(), t
            excused |= differs
        regime = particles["regimes"][t].cpu().numpy()
        assert regime.dtype == np.int32 and np.array_equal(regime[:, K - 1], reference[t])          # the reference in slot K-1
        differs = (regime != want["regimes"][t]).any(axis=1)
        assert not (differs & ~excused).any(), t
        excused |= differs
        keep = ~excused
        mean_error = np.linalg.norm(particles["means"][t].cpu().numpy() - want["means"][t], axis=-1)[keep]
        cov_error = np.linalg.norm(contract.unpack(particles["covariances"][t].cpu().numpy() - want["covariances"][t], D), 2,
                                   axis=(-2, -1))[keep]
        weight_error = np.abs(particles["log_weights"][t].cpu().numpy() - want["log_weights"][t])[keep]
        assert (mean_error <= want["tolerances"]["means"][t]).all(), t
        assert (cov_error <= want["tolerances"]["covariances"][t]).all(), t
        assert (weight_error <= want["tolerances"]["log_weights"][t]).all(), t
    last = want["margins"][T - 1] <= 4.0 * (want["tolerances"]["log_weights"][T - 1] + rounding)
    count += int(last.sum())
    excused |= last
    for t in range(T):
        keep = ~excused
        assert np.array_equal(particles["indices"][t].cpu().numpy()[keep], want["indices"][t][keep]), t
        assert path[t].dtype == torch.int32 and np.array_equal(path[t].cpu().numpy()[keep], want["path"][t][keep]), t
    draws = (T - 1) * B * K + B
    print("excused draws", count, "of", draws, "rows excused", int(excused.sum()), "of", B)
    assert count <= 0.001 * draws


def test_seeds_the_reference_slot_and_the_smoother_takes_the_paths(hip_device):
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 6, 4, 16, 3, 4, 2
    ops, _, _, reference, _, _ = sweep_case(T, B, K, M, D, Dy, 3)
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=4)
    reference = [_dev(r, hip_device) for r in reference]
    torch.manual_seed(11)
    first, particles = rao_blackwell.conditional_switching_filter(observations, model, K, reference, return_particles=True)
    torch.manual_seed(11)
    again = rao_blackwell.conditional_switching_filter(observations, model, K, reference)
    torch.manual_seed(12)
    other = rao_blackwell.conditional_switching_filter(observations, model, K, reference)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not all(torch.equal(a, b) for a, b in zip(first, other))
    assert all(torch.equal(particles["regimes"][t][:, K - 1], reference[t]) for t in range(T))     # bitwise
    rows = torch.arange(B, device=hip_device)
    assert all(torch.equal(first[t], particles["regimes"][t][rows, particles["indices"][t]]) for t in range(T))
    one = rao_blackwell.conditional_switching_filter(observations, model, 1, reference)
    assert all(torch.equal(a, b) for a, b in zip(one, reference))
    torch.manual_seed(13)
    np.random.seed(13)
    out = rao_blackwell.switching_particle_gibbs(observations, model, K, 5, burn_in=1)
    assert all(r.shape == (B, 4) and r.dtype == torch.int32 for r in out["regimes"])
    assert out["smoothed_regime_probabilities"].shape == (T, B, M)
    smoothed = rao_blackwell.switching_state_smooth(observations, model, out["regimes"])
    assert smoothed["smoothed_mean"].shape == (T, B, D) and bool(torch.isfinite(smoothed["smoothed_mean"]).all())
    filtered = rao_blackwell.conditional_kalman_filter(observations, model, out["regimes"])
    assert filtered["log_likelihood"].shape == (B, 4)


def test_invariance_and_mixing_against_the_enumeration(hip_device):
    """The CPU file's invariance check with fresh device uniforms: 8192 references from the exact joint law, ONE sweep each
    with K = 3, with and without ancestor sampling: every sequence's and every (t, regime) marginal's frequency within five
    binomial standard errors of its exact probability.  Then mixing from the worst start (all regimes 0): K = 8, 30 sweeps
    with ancestor sampling, the last sweep's marginals within the same bound of `exact_regime_marginals`."""
    from aesmc_amd import rao_blackwell
    ops, series, sequences, probabilities = invariance_case()
    T = len(series)
    model = _torch_model(ops, hip_device)
    observations = [_dev(np.broadcast_to(y, (CHAINS, 1)).copy(), hip_device) for y in series]
    for ancestor_sampling in (True, False):
        rng = np.random.default_rng(380 + int(ancestor_sampling))
        start = sequences[rng.choice(len(sequences), size=CHAINS, p=probabilities)]
        reference = [_dev(start[:, t].astype(np.int32), hip_device) for t in range(T)]
        torch.manual_seed(38 + int(ancestor_sampling))
        path = rao_blackwell.conditional_switching_filter(observations, model, 3, reference,
                                                          ancestor_sampling=ancestor_sampling)
        paths = np.stack([p.cpu().numpy() for p in path])
        assert_within_five_standard_errors(paths, sequences, probabilities,
                                           "device, " + ("ancestor sampling" if ancestor_sampling else "plain"))
    torch.manual_seed(39)
    zeros = [torch.zeros(CHAINS, dtype=torch.int32, device=hip_device) for _ in range(T)]
    out = rao_blackwell.switching_particle_gibbs(observations, model, 8, 30, reference=zeros, burn_in=29)
    marginals = contract.exact_regime_marginals(ops, series)
    worst = 0.0
    for t in range(T):
        for regime in range(2):
            p = marginals[t, regime]
            frequency = float((out["regimes"][t][:, 0] == regime).double().mean())
            allowed = 5.0 * np.sqrt(p * (1.0 - p) / CHAINS)
            worst = max(worst, abs(frequency - p) / allowed)
            assert abs(frequency - p) <= allowed, (t, regime, frequency, p)
    print("mixing: largest deviation over its allowance", worst)
