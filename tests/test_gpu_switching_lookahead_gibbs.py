"""Look-ahead particle Gibbs on the regimes of a switching linear-Gaussian model on the device: kernel K48
(aesmc_switching_lookahead_conditional_ancestor_index and its masked form) against its NumPy contract
(aesmc_amd/testing/switching_lookahead_gibbs.py) index for index and against the composition of K32 and K37 it replaces, its
bad rows, the entry K49 (aesmc_switching_kalman_conditional_draw) against K33 and K38 bit for bit, the C ABI's refusals, and
`conditional_switching_filter(..., lookahead=True)` / `switching_particle_gibbs(..., lookahead=True)` end to end: replayed
against the contract's pass, and the invariance and mixing of the chain against the enumeration of all regime sequences."""
import ctypes

import numpy as np
import pytest
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_lookahead_gibbs as lookahead
from aesmc_amd.testing import switching_missing as missing
from tests.test_gpu_switching_gibbs import _dev, _provider, _torch_model
from tests.test_switching_gibbs_contract import CHAINS, assert_within_five_standard_errors, invariance_case, sweep_case

pytestmark = pytest.mark.gpu

FUSED_CAP = "fused cap"            # K: the fused launch's cap for the model; "+1": one more, which only the composition takes
# (B, K, M, D, Dy, information depth, float32 y, ancestor sampling, masked, seed).  K: one lane; one free slot; two; a partial
# wavefront, a full one, the first size on 256 lanes, several particles per lane; the cap and the cap + 1 of a small and of an
# 8-wide model.  (D, Dy): every pad of either.  The seeds are chosen on the CPU: see the test.
CASES = [(1, 1, 1, 1, 1, 1, False, True, False, 0),
         (3, 2, 2, 2, 3, 1, True, True, False, 0),
         (3, 3, 2, 3, 2, 3, False, False, False, 0),
         (3, 63, 2, 4, 4, 1, False, True, False, 0),
         (1, 64, 16, 5, 8, 3, True, True, False, 0),
         (3, 65, 2, 8, 5, 1, False, True, False, 0),
         (3, 257, 2, 8, 8, 3, False, True, False, 0),
         (1, 257, 16, 8, 8, 1, True, False, False, 0),
         (3, 7, 2, 2, 3, 1, False, True, True, 0),
         (3, 64, 2, 4, 4, 1, False, False, True, 0),
         (3, 65, 3, 8, 8, 3, True, True, True, 0),
         (1, FUSED_CAP, 16, 2, 2, 1, False, True, False, 0),
         (1, FUSED_CAP + "+1", 16, 2, 2, 1, False, True, False, 0),
         (1, FUSED_CAP, 16, 8, 8, 1, False, True, False, 0),
         (1, FUSED_CAP + "+1", 16, 8, 8, 1, False, True, False, 0)]


def fused_cap(M, D, Dy):
    """The formula of csrc/switching_lookahead_conditional.hip's header (the library's own value is compared in the test)."""
    pad = lambda n: 2 if n <= 2 else 4 if n <= 4 else 8
    P, Q = pad(D), pad(Dy)
    T = P * (P + 1) // 2
    fixed = T + P + 30 + M * M + M * (P * P + 2 * P + Q * P + 2 * Q) + (256 * T if P == 8 else 0) + 256 * M
    return min(8192 if D <= 4 else 4096, (160 * 1024 // 8 - fixed) // 2)


def step_case(B, K, M, D, Dy, steps, y_is_float, ancestor_sampling, masked, seed):
    """The operands of one look-ahead conditional resampling step, NumPy: `example_backward_step`'s stored particles and
    observation, (F, lam) from `steps` information steps along one trajectory per row; under a mask row 0 measured
    everything, row 1 part (where Dy > 1), the last row nothing."""
    if isinstance(K, str):
        K = fused_cap(M, D, Dy) + (1 if K.endswith("+1") else 0)
    model, regime_next, info, y, particles, _ = contract.example_backward_step(
        B, K, 1, M, D, Dy, steps=steps, observation_dtype=np.float32 if y_is_float else np.float64, seed=seed)
    observed = None
    if masked:
        observed = np.ones((B, Dy), dtype=bool)
        observed[1, ::2] = False
        observed[B - 1] = False
        _, lam, _, F, flags, margin = missing.switching_information_step(model, regime_next, info, y, observed)
    else:
        _, lam, _, F, flags, margin = contract.switching_information_step(model, regime_next, info, y)
    assert flags == 0 and margin > 1e-13
    u = np.random.default_rng([seed, B, K, M, D, Dy, steps, 48]).uniform(size=(B, K))
    with np.errstate(divide="ignore"):
        log_Pi = np.log(model["Pi"])
    F, lam = (F[:, 0].copy(), lam[:, 0].copy()) if ancestor_sampling else (None, None)
    return dict(model=model, log_Pi=log_Pi, particles=particles, y=y, u=u, regime_next=regime_next[:, 0].copy(), F=F, lam=lam,
                observed=observed, K=K)


def margins_exceed_bounds(want, K):
    """From the contract alone: no free draw lies within what first-stage weights off by their bounds can move the normalised
    running sum (a weight off by e moves it by at most exp(2 e) - 1 <= 4 e) plus the rounding of K summed weights (8 K u);
    no pinned draw within the same of its scores' bound."""
    _, _, _, _, margins, score_bound, (bound_w, _) = want
    rounding = 8 * K * contract.UNIT
    free = (margins[:, :K - 1] > 4.0 * bound_w.max(axis=1, keepdims=True) + rounding).all()
    pinned = (margins[:, K - 1] > 4.0 * score_bound + rounding).all()
    return bool(free and pinned)


def device_step(provider, device, case, fused, **changed):
    values = dict(case, **changed)
    ops = {name: _dev(value, device) for name, value in values["model"].items()}
    return provider.switching_lookahead_conditional_ancestor_index(
        ops, _dev(values["log_Pi"], device), tuple(_dev(part, device) for part in values["particles"]), _dev(values["y"], device),
        _dev(values["u"], device), _dev(values["regime_next"], device), _dev(values["F"], device), _dev(values["lam"], device),
        observed=_dev(values["observed"], device), fused=fused)


def contract_step(case, **changed):
    values = dict(case, **changed)
    return lookahead.lookahead_conditional_ancestor_index(values["model"], values["log_Pi"], values["particles"], values["y"],
                                                          values["u"], values["regime_next"], values["F"], values["lam"],
                                                          observed=values["observed"])


@pytest.mark.parametrize("B,K,M,D,Dy,steps,y_is_float,ancestor_sampling,masked,seed", CASES)
def test_the_fused_launch_equals_the_contract_and_the_composition(hip_device, B, K, M, D, Dy, steps, y_is_float,
                                                                  ancestor_sampling, masked, seed):
    """First the margins, from the contract alone (a property of the seeds).  Then every index is equal — no draw is excused —
    and the first-stage log-weights and cumulative rows lie within `switching_lookahead_bound`.  Then the composition (K32 or
    K40, K37 twice, one torch.where) gives the same indices.  One past the cap only the composition runs."""
    provider = _provider()
    beyond = isinstance(K, str) and K.endswith("+1")
    case = step_case(B, K, M, D, Dy, steps, y_is_float, ancestor_sampling, masked, seed)
    K = case["K"]
    cap = provider.switching_lookahead_conditional_max_particles(M, D, Dy)
    assert cap == fused_cap(M, D, Dy) and (K == cap + 1 if beyond else K <= cap)
    want = contract_step(case)
    idx, log_w, cdf, flags, margins, score_bound, (bound_w, bound_c) = want
    assert flags == 0
    print("smallest free margin", margins[:, :K - 1].min() if K > 1 else None, "smallest pinned margin", margins[:, K - 1].min(),
          "largest bounds", bound_w.max(), bound_c.max(), score_bound.max())
    assert margins_exceed_bounds(want, K)
    if masked:      # the row that measured nothing: equal first-stage weights
        assert np.abs(log_w[B - 1]).max() < 1e-14
    composed = device_step(provider, hip_device, case, False)
    assert provider.read_flags(hip_device) == 0
    if beyond:
        with pytest.raises(ValueError, match="fused=True"):
            device_step(provider, hip_device, case, True)
        got = device_step(provider, hip_device, case, None)      # (None: the cap decides — the composition)
    else:
        got = device_step(provider, hip_device, case, True)
    assert provider.read_flags(hip_device) == 0
    assert got[0].dtype == torch.int64 and got[0].shape == (B, K) and got[2].shape == (B, K, M)
    assert torch.equal(got[0].cpu(), torch.from_numpy(idx))
    assert torch.equal(got[0], composed[0])
    for mine in (got, composed):
        assert (np.abs(mine[1].cpu().numpy() - log_w) <= bound_w).all()
        assert (np.abs(mine[2].cpu().numpy() - cdf) <= bound_c).all()
    if not ancestor_sampling:
        assert bool((got[0][:, K - 1] == K - 1).all())


def test_bad_rows_leave_every_other_row_as_it_was(hip_device):
    provider = _provider()
    B, K, M, D, Dy = 5, 300, 4, 5, 3
    case = step_case(B, K, M, D, Dy, 2, False, True, False, 0)
    clean = [part.cpu().numpy() for part in device_step(provider, hip_device, case, True)]
    assert provider.read_flags(hip_device) == 0

    def both(flags, **changed):
        want = contract_step(case, **changed)
        assert want[3] == flags
        for fused in (True, False):
            got = [part.cpu().numpy() for part in device_step(provider, hip_device, case, fused, **changed)]
            assert provider.read_flags(hip_device) == flags, fused
            assert np.array_equal(got[0], want[0]), fused
            assert np.array_equal(np.isnan(got[1]), np.isnan(want[1])) and np.array_equal(np.isnan(got[2]), np.isnan(want[2]))
        return got

    # a stored regime outside [0, M): its first-stage weight is NaN, every slot of its row is K
    regime = case["particles"][0].copy()
    regime[0, 4], regime[4, 256] = M, -1
    got = both(contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT,
               particles=(regime, case["particles"][1], case["particles"][2]))
    assert (got[0][[0, 4]] == K).all() and np.array_equal(got[0][1:4], clean[0][1:4])
    assert np.isnan(got[1][0, 4]) and np.isnan(got[2][4, 256]).all() and np.array_equal(got[1][1:4], clean[1][1:4])
    # a pinned regime outside [0, M): slot K-1 of its row alone
    outside = case["regime_next"].copy()
    outside[2] = M
    got = both(contract.FLAG_INDEX_OUT_OF_RANGE | contract.FLAG_NAN_LOG_WEIGHT, regime_next=outside)
    assert got[0][2, K - 1] == K and np.array_equal(got[0][:, :K - 1], clean[0][:, :K - 1])
    assert np.array_equal(np.delete(got[0], 2, 0), np.delete(clean[0], 2, 0)) and np.array_equal(got[1], clean[1])
    # a zero column of Pi into s'_t: the first-stage weights stay finite, only slot K-1 of the rows that enter it fails
    Pi = np.array(case["model"]["Pi"])
    Pi[:, case["regime_next"][0]] = 0.0
    Pi /= Pi.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        got = both(contract.FLAG_DEGENERATE_ROW, log_Pi=np.log(Pi))
    hit = case["regime_next"] == case["regime_next"][0]
    assert (got[0][hit, K - 1] == K).all() and (got[0][:, :K - 1] < K).all() and (got[0][~hit, K - 1] < K).all()
    # a pivot that is not positive under a regime of positive prior: NaN first-stage weights, the whole row
    cov = case["particles"][2].copy()
    cov[3] = 0.0
    broken = dict(case["model"], r=np.zeros_like(case["model"]["r"]), q=np.zeros_like(case["model"]["q"]))
    got = both(contract.FLAG_NAN_LOG_WEIGHT, model=broken, particles=(case["particles"][0], case["particles"][1], cov))
    assert (got[0][3] == K).all() and np.isnan(got[1][3]).all()


@pytest.mark.parametrize("later,index", [(False, "none"), (True, "unsorted")])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,K,M,D,Dy", [(1, 1, 1, 1, 1), (3, 7, 2, 2, 3), (2, 65, 3, 8, 8), (2, 300, 4, 5, 3)])
def test_the_conditional_draw_is_k33_and_k38_bit_for_bit(hip_device, B, K, M, D, Dy, masked, later, index):
    """Slots 0 .. K-2 of K49 equal K33 on the same inputs bitwise, slot K-1 equals K38's bitwise: regime, mean, covariance and
    log-likelihood.  K31, K33 and K38 through their own entries are still their contracts' in every slot (regimes equal, the
    rest within the bounds), and so is K49 its own."""
    provider = _provider()
    model, state, idx, uniforms, y = contract.example_step(B, K, M, D, Dy, index=index, later=later)
    observed = None
    if masked:
        observed = np.ones((B, Dy), dtype=bool)
        observed[B - 1, ::2] = False
    prior = np.log(model["Pi"]) if later else np.log(model["pi0"])
    _, cdf, flags = contract.switching_lookahead(model, prior, state, y, K)
    assert flags == 0
    pinned = np.random.default_rng([B, K, M, 49]).integers(0, M, B).astype(np.int32)
    ops = {name: _dev(value, hip_device) for name, value in model.items()}
    dev_state = None if state is None else tuple(_dev(part, hip_device) for part in state)
    args = (ops, dev_state, _dev(idx, hip_device), _dev(uniforms, hip_device))
    mask = {} if observed is None else {"observed": _dev(observed, hip_device)}
    got = provider.switching_kalman_conditional_draw(*args, _dev(cdf, hip_device), _dev(pinned, hip_device), _dev(y, hip_device),
                                                     **mask)
    free = provider.switching_kalman_draw(*args, _dev(cdf, hip_device), _dev(y, hip_device), **mask)
    last = provider.switching_kalman_conditional_step(*args, _dev(pinned, hip_device), _dev(y, hip_device), **mask)
    assert provider.read_flags(hip_device) == 0
    assert torch.equal(got[0][:, K - 1].cpu(), torch.from_numpy(pinned))
    for part, a, b in zip(got, free, last):
        assert torch.equal(part[:, :K - 1], a[:, :K - 1]) and torch.equal(part[:, K - 1], b[:, K - 1])
    plain = provider.switching_kalman_step(*args, _dev(y, hip_device), **mask)      # K31 through its own entry
    assert provider.read_flags(hip_device) == 0
    if observed is None:
        contracts = [
            (plain, contract.switching_kalman_step(model, state, idx, uniforms, y),
             contract.switching_kalman_step_bound(model, state, idx, uniforms, y)),
            (free, contract.switching_kalman_draw(model, state, idx, uniforms, cdf, y),
             contract.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y)),
            (last, contract.switching_kalman_conditional_step(model, state, idx, uniforms, pinned, y),
             contract.switching_kalman_conditional_step_bound(model, state, idx, uniforms, pinned, y))]
    else:
        contracts = [
            (plain, missing.switching_kalman_step(model, state, idx, uniforms, y, observed),
             missing.switching_kalman_step_bound(model, state, idx, uniforms, y, observed)),
            (free, missing.switching_kalman_draw(model, state, idx, uniforms, cdf, y, observed),
             missing.switching_kalman_draw_bound(model, state, idx, uniforms, cdf, y, observed)),
            (last, missing.switching_kalman_conditional_step(model, state, idx, uniforms, pinned, y, observed),
             missing.switching_kalman_conditional_step_bound(model, state, idx, uniforms, pinned, y, observed))]
    contracts.append((got, lookahead.switching_kalman_conditional_draw(model, state, idx, uniforms, cdf, pinned, y,
                                                                        observed=observed),
                      lookahead.switching_kalman_conditional_draw_bound(model, state, idx, uniforms, cdf, pinned, y,
                                                                        observed=observed)))
    for mine, want, bounds in contracts:      # K31, K33, K38 and K49: every slot's regime equal, the rest within the bounds
        assert want[4] == 0 and np.array_equal(mine[0].cpu().numpy(), want[0])
        for part, expected, bound in zip(mine[1:], want[1:4], bounds):
            assert (np.abs(part.cpu().numpy() - expected) <= bound).all()
    # a pinned regime outside [0, M): that slot alone
    bad = pinned.copy()
    bad[B - 1] = M
    out = provider.switching_kalman_conditional_draw(*args, _dev(cdf, hip_device), _dev(bad, hip_device), _dev(y, hip_device),
                                                     **mask)
    assert provider.read_flags(hip_device) == contract.FLAG_INDEX_OUT_OF_RANGE
    assert int(out[0][B - 1, K - 1]) == 0 and bool(torch.isnan(out[3][B - 1, K - 1]))
    keep = torch.ones((B, K), dtype=torch.bool, device=hip_device)
    keep[B - 1, K - 1] = False
    for part, reference in zip(out, got):
        assert torch.equal(part[keep], reference[keep])


def test_the_abi_refuses_bad_arguments_without_a_launch(hip_device):
    """Device pointers: a refusal must leave the outputs as they were."""
    from aesmc_amd import _lib
    lib = _lib.load()
    B, K, M, D, Dy = 2, 7, 2, 2, 1
    case = step_case(B, K, M, D, Dy, 2, False, True, False, 0)
    ops = {name: _dev(value, hip_device) for name, value in case["model"].items()}
    keys = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
    block = lambda **kw: _lib.SwitchingModel(*([ops[name].data_ptr() for name in keys] + [kw.get("M", M), kw.get("D", D),
                                                                                          kw.get("Dy", Dy)]))
    names = ("log_Pi", "regime", "mean", "cov", "y", "u", "regime_next", "F", "lam")
    values = dict(case, regime=case["particles"][0], mean=case["particles"][1], cov=case["particles"][2])
    operands = {name: _dev(values[name], hip_device) for name in names}
    observed = torch.ones((B, Dy), dtype=torch.bool, device=hip_device)
    outs = {"idx": torch.full((B, K), 7, dtype=torch.int64, device=hip_device),
            "log_weight": torch.full((B, K), 7.0, dtype=torch.float64, device=hip_device),
            "cdf": torch.full((B, K, M), 7.0, dtype=torch.float64, device=hip_device)}
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(masked=False, model=None, B=B, K=K, dtype=1, **changed):
        given = dict(operands, **outs)
        given.update(changed)
        model = block() if model is None else model
        head = [dtype, ctypes.byref(model)] + [ptr(given[name]) for name in names[:5]]
        tail = [ptr(given[name]) for name in names[5:]] + [ptr(given["idx"]), ptr(given["log_weight"]), ptr(given["cdf"]), None,
                                                           B, K, None]
        if masked:
            return lib.aesmc_switching_masked_lookahead_conditional_ancestor_index(*(head + [ptr(given.get("observed", observed))]
                                                                                     + tail))
        return lib.aesmc_switching_lookahead_conditional_ancestor_index(*(head + tail))

    for masked in (False, True):
        for name in ("log_Pi", "regime", "mean", "cov", "y", "u", "idx", "log_weight", "cdf"):
            assert call(masked, **{name: None}) == 1, name
        assert call(masked, F=None) == 1 and call(masked, lam=None) == 1 and call(masked, regime_next=None) == 1
        assert call(masked, idx=operands["u"]) == 1 and call(masked, cdf=outs["log_weight"]) == 1 and call(masked, dtype=5) == 1
        assert call(masked, K=-1) == 1 and call(masked, model=block(M=0)) == 1
        assert call(masked, model=block(D=9)) == 2 and call(masked, model=block(M=17)) == 2
        assert call(masked, K=fused_cap(M, D, Dy) + 1) == 2 and call(masked, B=1 << 31) == 2
        assert call(masked, B=0) == 0 and call(masked, K=0) == 0
    assert call(True, observed=None) == 1
    state = [operands["regime"], operands["mean"], operands["cov"]]
    index = torch.zeros((B, K), dtype=torch.int64, device=hip_device)
    rows = torch.ones((B, K, M), dtype=torch.float64, device=hip_device)
    step_outs = [torch.full((B, K), 7, dtype=torch.int32, device=hip_device)] + \
        [torch.full(shape, 7.0, dtype=torch.float64, device=hip_device) for shape in ((B, K, D), (B, K, 3), (B, K))]

    def step(model=None, state=state, idx=index, uniforms=operands["u"], cdf=rows, pinned=operands["regime_next"],
             y=operands["y"], outs=step_outs, B=B, K=K, dtype=1):
        model = block() if model is None else model
        return lib.aesmc_switching_kalman_conditional_draw(dtype, ctypes.byref(model), *[ptr(t) for t in state], ptr(idx),
                                                           ptr(uniforms), ptr(cdf), ptr(pinned), ptr(y),
                                                           *[ptr(t) for t in outs], None, B, K, None)

    assert step(pinned=None) == 1 and step(cdf=None) == 1 and step(uniforms=None) == 1 and step(y=None) == 1
    assert step(dtype=5) == 1 and step(state=[None] + state[1:]) == 1 and step(outs=step_outs[:3] + [None]) == 1
    assert step(outs=[state[0]] + step_outs[1:]) == 1 and step(pinned=step_outs[0]) == 1 and step(cdf=step_outs[3]) == 1
    assert step(B=-1) == 1
    assert step(model=block(D=9)) == 2 and step(model=block(M=17)) == 2 and step(B=1 << 16, K=1 << 16) == 2
    assert step(B=0) == 0 and step(K=0) == 0
    torch.cuda.synchronize()
    assert bool((outs["idx"] == 7).all()) and bool((outs["log_weight"] == 7).all()) and bool((outs["cdf"] == 7).all())
    assert all(bool((t == 7).all()) for t in step_outs)


SWEEP_SEEDS = {(True, False): 0, (False, False): 0, (True, True): 0}


@pytest.mark.parametrize("ancestor_sampling,masked", sorted(SWEEP_SEEDS))
def test_a_whole_sweep_on_replayed_uniforms_equals_the_contracts_pass(hip_device, ancestor_sampling, masked):
    """T = 6, K = 8, B = 4, M = 3, D = 4, Dy = 2.  A draw is excused where its contract margin is within what its inputs,
    off by the contract's propagated tolerances, can move it: 4 e of the normalised running sums (e: the first-stage
    weights' tolerance, the pinned scores' bound plus it) and e of a posterior row (its tolerance).  The number of excused
    draws is reported and, for the chosen seeds, asserted 0: every ancestor, regime, index and the path are then equal, and
    means, covariances and first-stage log-weights lie within the tolerances."""
    from aesmc_amd import rao_blackwell
    T, B, K, M, D, Dy = 6, 4, 8, 3, 4, 2
    seed = SWEEP_SEEDS[(ancestor_sampling, masked)]
    ops, _, _, reference, uniforms, regime_u = sweep_case(T, B, K, M, D, Dy, seed)
    model = _torch_model(ops, hip_device)
    observations = model.simulate(T, B, seed=seed + 1)
    observed = None
    if masked:
        observed = [None if t % 3 == 0 else missing.example_mask(B, Dy, variant=t, seed=seed) for t in range(T)]
        observed[2] = np.zeros((B, Dy), dtype=bool)      # a step where nothing was measured
    ys = [y.cpu().numpy() for y in observations]
    want = lookahead.lookahead_conditional_switching_pass(ys, ops, K, reference, uniforms, regime_u,
                                                          ancestor_sampling=ancestor_sampling, observed=observed)
    assert want["flags"] == 0
    rounding = 8 * K * contract.UNIT
    count = 0
    for t in range(T):
        if t > 0:
            carried = want["tolerances"]["first_stage_log_weights"][t] + rounding
            margins = want["margins"][t - 1]
            count += int((margins[:, :K - 1] <= 4.0 * carried).sum())
            count += int((margins[:, K - 1] <= 4.0 * (carried + want["score_bounds"][t - 1])).sum())
        count += int(want["regime_margins"][t] <= want["tolerances"]["cdf"][t])
    count += int((want["margins"][T - 1] <= rounding).sum())
    print("excused draws", count, "of", (T - 1) * B * K + T * B * (K - 1) + B)
    assert count == 0
    dev = lambda blocks: [_dev(block, hip_device) for block in blocks]
    path, particles = rao_blackwell.conditional_switching_filter(
        observations, model, K, dev(reference), ancestor_sampling=ancestor_sampling, uniforms=dev(uniforms),
        regime_uniforms=dev(regime_u), return_particles=True, lookahead=True,
        observed=None if observed is None else [None if o is None else _dev(o, hip_device) for o in observed])
    assert len(particles["first_stage_log_weights"]) == T
    for t in range(T):
        if t > 0:
            assert np.array_equal(particles["ancestral_indices"][t - 1].cpu().numpy(), want["ancestral_indices"][t - 1]), t
        regime = particles["regimes"][t].cpu().numpy()
        assert regime.dtype == np.int32 and np.array_equal(regime[:, K - 1], reference[t]) and np.array_equal(regime, want["regimes"][t])
        mean_error = np.linalg.norm(particles["means"][t].cpu().numpy() - want["means"][t], axis=-1)
        cov_error = np.linalg.norm(contract.unpack(particles["covariances"][t].cpu().numpy() - want["covariances"][t], D), 2,
                                   axis=(-2, -1))
        weight_error = np.abs(particles["first_stage_log_weights"][t].cpu().numpy() - want["first_stage_log_weights"][t])
        assert (mean_error <= want["tolerances"]["means"][t]).all(), t
        assert (cov_error <= want["tolerances"]["covariances"][t]).all(), t
        assert (weight_error <= want["tolerances"]["first_stage_log_weights"][t]).all(), t
        assert bool((particles["log_weights"][t] == 0).all())
        assert np.array_equal(particles["indices"][t].cpu().numpy(), want["indices"][t]), t
        assert path[t].dtype == torch.int32 and np.array_equal(path[t].cpu().numpy(), want["path"][t]), t


def test_invariance_and_mixing_against_the_enumeration(hip_device):
    """The CPU file's invariance check with fresh device uniforms: 8192 references from the exact joint law, ONE look-ahead
    sweep each with K = 3, with and without ancestor sampling: every sequence's and every (t, regime) marginal's frequency
    within five binomial standard errors of its exact probability.  Then mixing from the worst start (all regimes 0): K = 8,
    30 look-ahead sweeps with ancestor sampling, the last sweep's marginals within the same allowance."""
    from aesmc_amd import rao_blackwell
    ops, series, sequences, probabilities = invariance_case()
    T = len(series)
    model = _torch_model(ops, hip_device)
    observations = [_dev(np.broadcast_to(y, (CHAINS, 1)).copy(), hip_device) for y in series]
    for ancestor_sampling in (True, False):
        rng = np.random.default_rng(490 + int(ancestor_sampling))
        start = sequences[rng.choice(len(sequences), size=CHAINS, p=probabilities)]
        reference = [_dev(start[:, t].astype(np.int32), hip_device) for t in range(T)]
        torch.manual_seed(48 + int(ancestor_sampling))
        path = rao_blackwell.conditional_switching_filter(observations, model, 3, reference,
                                                          ancestor_sampling=ancestor_sampling, lookahead=True)
        paths = np.stack([p.cpu().numpy() for p in path])
        assert (paths != start.T).any()
        assert_within_five_standard_errors(paths, sequences, probabilities,
                                           "device look-ahead, " + ("ancestor sampling" if ancestor_sampling else "plain"))
    torch.manual_seed(49)
    zeros = [torch.zeros(CHAINS, dtype=torch.int32, device=hip_device) for _ in range(T)]
    out = rao_blackwell.switching_particle_gibbs(observations, model, 8, 30, reference=zeros, burn_in=29, lookahead=True)
    marginals = contract.exact_regime_marginals(ops, series)
    worst = 0.0
    for t in range(T):
        for regime in range(2):
            p = marginals[t, regime]
            frequency = float((out["regimes"][t][:, 0] == regime).double().mean())
            allowed = 5.0 * np.sqrt(p * (1.0 - p) / CHAINS)
            worst = max(worst, abs(frequency - p) / allowed)
            assert abs(frequency - p) <= allowed, (t, regime, frequency, p)
    print("look-ahead mixing: largest deviation over its allowance", worst)
