"""K1 (logweight_lse.hip) and K7 (particle_summary.hip) against the float64 contract of aesmc_amd/testing/reductions.py, in
every form their launchers can choose, on inputs under which no particle, tile, slice or tail can be wrong unnoticed.

Measured on the MI355X (gfx950), the worst case per family.  `cases` counts the comparisons made, `exact` those among
them held to an error of exactly 0 (`one_hot`); e_ref, limit and error are the largest over the others, err/lim the
largest ratio and the case it belongs to.  In float64 the limit is the derived bound and e_ref does not apply.

  family                 dtype    cases  exact      e_ref      limit      error  err/lim  worst case
  K7 log_ess             float32    262     42   4.32e-07   3.45e-06   7.95e-07    0.417  general4-5x300x2 wide
  K7 mean                float32    247     38   3.12e-07   2.49e-06   5.88e-07    0.308  general4-5x300x2 wide
  K7 second              float32    247     38   3.01e-07   2.40e-06   9.66e-07    0.507  general16-1x1024x2052 flat
  K7 log_ess             float64    262     42          -   3.39e-12   2.30e-15    0.025  ess-only-700x40 wide
  K7 mean                float64    247     38          -   9.75e-13   2.47e-15    0.026  general4-1x40x1030 wide
  K7 second              float64    247     38          -   9.75e-13   6.30e-15    0.024  general4-1x40x1030 wide
  K7 special log_ess     float32     24      0   1.39e-07   1.91e-06   1.39e-07    0.073  small-4x1537x5 every_second_minus_inf@1
  K7 special mean        float32     24      0   2.19e-08   1.91e-06   2.28e-08    0.012  general16-4x1540x20 every_second_minus_inf@1
  K7 special second      float32     24      0   9.17e-08   1.91e-06   3.40e-07    0.179  general4-4x1600x2 every_second_minus_inf@2
  K7 special (3 outputs) float64     72      0          -   1.13e-12   2.30e-15    0.003  small-4x1537x5 minus_inf_slice@2
  K1 forward lse         float32    209     65   6.18e-07   4.94e-06   6.34e-07    0.234  3x256 flat:a+b
  K1 forward lse         float64    209     65          -   1.84e-12   1.42e-15    0.013  5x63 minus_inf_stretch:a+b-c
  K1 accumulate lse      float32    157     39   6.33e-07   5.06e-06   6.48e-07    0.217  2x4099 minus_inf_stretch
  K1 accumulate lse      float64    157     39          -   1.84e-12   1.11e-15    0.013  5x63 offset_up
  K1 backward g          float32    219     39   5.88e-07   4.70e-06   5.88e-07    0.125  2048x1024 flat/as-drawn:+lse
  K1 backward g          float64    219     39          -   2.68e-12   4.36e-16    0.115  6x255 descending:+lse
  K1 non-finite lse, fwd float32      5      0   4.25e-07   3.40e-06   3.56e-07    0.125  6x257 (the finite rows beside the special ones)
  K1 non-finite lse, fwd float64      5      0          -   9.32e-13   4.44e-16    0.006  6x257
  K1 non-finite lse, bwd both        60     60   5 forms x 2 dtypes x 3 gradient combinations x (g, -g): every convention exact
  fused step lse (x4)    float32     32     16   2.75e-09   1.91e-06   2.75e-09    0.001  2x4096 probes_inf (every entry alike)
  fused step lse (x4)    float64     32     16          -   4.48e-13   0.00e+00    0.000
  one-hot sweeps         both        24     24   K7: 4 shapes x 2 dtypes x {-1e4, -inf}; K1: 2 x 2 x 2 — every output exact

No case needed a redraw (0 of 2984 comparisons; the largest 8 e_ref is 5.1e-06 against the cap of 1e-5).  The ascending
rows, where LseState rescales its sum at every push, stay at 0.13 of their float32 limit.  No kernel bug was found.  (That
the module can fail was checked once by hand: a build whose kernels leave out the last particle of a row fails every K7
case and every non-vector K1 case here.)

Two departures from the profiles as first written, both in reductions.py: `wide` is clipped at +-36 in float32 (beyond,
exp(lw - lse) is a subnormal float32 and a relative metric without a floor has nothing to hold on to), and K1's backward
gets lw and lse on a grid of 2^-10, so that the float32 difference lw - lse is exact — except under `flat`, which also runs
as drawn (the `/as-drawn` rows above), where that shared rounding stays below the conditioning cap.

How a case is held.  Every case asserts the form it means to run from the launcher's own record
(aesmc_test_last_particle_summary_form / aesmc_test_last_logweight_form, decoded in tests/reduction_cases.py) and then
compares with the contract under a metric without hiding places:

  * lse, log_ess:          |got - want| / max(1, |want|)  (K1's rows are centred so that |lse| <= 1/2: an absolute error);
  * mean, second moment:   |got - want| / sum_k w_k |v_k|  (resp. sum_k w_k v_k^2) per output element, no floor; exactly 0
                           where that magnitude is 0;
  * K1's gradient:         per particle, |g - want| / (|grad_lse| exp(lw - lse) + |grad_lw|); exactly 0 where that is 0;
  * lw and total of K1:    bit for bit (IEEE additions).

The limit: float64 — the contract's derived bound (eps64 (K + 96) per sum; reductions.py).  float32 — not a constant:
each case measures e_ref, the error of eager float32 PyTorch on the device for the same expression on the same inputs
under the same metric (torch.logsumexp, softmax-weighted sums, grad_lse[:, None] * exp(lw - lse[:, None]) + grad_lw),
and allows max(8 e_ref, 16 eps32): another fixed summation order and the hardware's exp, the rule of
tests/gradient_checks.py.  A case whose 8 e_ref exceeds 1e-5 is ill-conditioned and its weights are drawn again (the
draw is printed and bounded); the factor never changes.  `one_hot` rows are held exactly in both dtypes.  That these
inputs have teeth — a particle left out, counted twice, a slice left out moves an output by >= 1e-4, ten times the cap —
is proved on the CPU by tests/test_reductions_contract.py for every (profile, shape) used here.

Every case prints a FIGURES line: family, case, dtype, profile, form, e_ref, limit, kernel error, draws.
"""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import reductions as R
from tests import reduction_cases as C

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


@pytest.fixture(scope="module")
def kernels(hip_device):
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _dev(array, device, shift=0):
    """The array on the device; with `shift`, as a contiguous view that many elements into a larger buffer (its base
    pointer is then not 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    if not shift:
        return t.to(device)
    buffer = torch.empty(t.numel() + shift, dtype=t.dtype, device=device)
    view = buffer[shift:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _host(t):
    return None if t is None else t.detach().cpu().numpy()


def _limit32(e_ref):
    return max(8.0 * e_ref, 16.0 * EPS32)


def _figures(family, case, dtype, profile, form, e_ref, limit, err, draws=1):
    print("FIGURES family={} case={} dtype={} profile={} form={} e_ref={:.3e} limit={:.3e} err={:.3e} draws={}".format(
        family, case, np.dtype(dtype).name, profile, form, e_ref, limit, err, draws))


def _hold(family, case, dtype, profile, form, errs, refs, bounds, draws=1):
    """errs / refs / bounds: per output, the kernel's error, eager float32's (None in float64) and the float64 bound."""
    for key, err in errs.items():
        if C.is_exact(profile) and bounds.get(key) != "limit":
            limit, e_ref = 0.0, 0.0
        elif dtype == np.float32:
            e_ref = refs[key]
            limit = _limit32(e_ref)
        else:
            e_ref, limit = 0.0, float(bounds[key + "_bound"])
        _figures(family + "/" + key, case, dtype, profile, form, e_ref, limit, err, draws)
        assert err <= limit, "{} {} {} {}: {} off by {:.3e}, limit {:.3e} (e_ref {:.3e})".format(
            family, case, np.dtype(dtype).name, profile, key, err, limit, e_ref)


# ---- K7 -------------------------------------------------------------------------------------------------------------------
def _summary_form(kernels):
    return C.summary_form(kernels._lib.aesmc_test_last_particle_summary_form())


def _assert_summary_form(kernels, case, with_values=True):
    form = _summary_form(kernels)
    want = case.form if with_values else {"kernel": C.GENERAL4, "S": case.S, "TX": 1, "sweeps": 1}
    for key, val in want.items():
        assert form[key] == val, "{}: {} is {}, meant {} ({})".format(case, key, form[key], val, form)
    return "k{kernel}{d}/S{S}/TX{TX}/x{sweeps}".format(d="d" if form["dense"] else "", **form)


def _eager_summary(lw, value):
    """Eager PyTorch in lw's dtype.  The row maximum is taken off first (an exact subtraction of neighbours): 2 lse(lw) -
    lse(2 lw) as written cancels two numbers of the offset's size, which is the expression's weakness and not a measure
    of what a summation order costs."""
    top = lw.max(1, keepdim=True).values
    x = lw - torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    log_ess = 2 * torch.logsumexp(x, 1) - torch.logsumexp(2 * x, 1)
    if value is None:
        return log_ess, None, None
    w = torch.softmax(lw, 1).reshape(lw.shape + (1,) * (value.dim() - 2))
    return log_ess, (w * value).sum(1), (w * value * value).sum(1)


def _summary_errors(got, lw, value):
    """Errors of (log_ess, mean, second) — host arrays or None — against the contract, with the float64 bounds."""
    want = R.particle_summary(lw, value)
    errs = {}
    if got[0] is not None:
        errs["log_ess"] = C.error_floor_one(got[0], want[0])
    if value is not None:
        sizes = R.summary_magnitudes(lw, value)
        if got[1] is not None:
            errs["mean"] = C.error_relative(got[1], want[1], sizes[0])
        if got[2] is not None:
            errs["second"] = C.error_relative(got[2], want[2], sizes[1])
    return errs


def _summary_bounds(lw):
    bound = float(R.summary_bound(lw).max())
    return {"log_ess_bound": float(R.log_ess_bound(lw).max()), "mean_bound": bound, "second_bound": bound}


def _summary_value(case, dtype, device):
    base, view = case.value()
    if view is None:
        return None, None
    base_dev = _dev(base.astype(dtype), device)
    value_dev = base_dev if case.view is None else case.view(base_dev)
    assert value_dev.shape == view.shape
    return view, value_dev


def _check_summary(kernels, device, case, dtype, profile, value, value_dev, wanted=(True, True, True)):
    """One profile on one case: weights drawn (again while ill-conditioned), launched, held.  Returns the outputs."""
    for draw in range(C.MAX_DRAWS):
        lw = C.weights(profile, case.B, case.K, dtype, C.case_seed(case, profile, draw), L=case.L)
        lw_dev = _dev(lw, device)
        refs = {}
        if dtype == np.float32:
            eager = [_host(t) for t in _eager_summary(lw_dev, value_dev)]
            refs = _summary_errors(eager, lw, value)
            if 8.0 * max(refs.values()) > C.CONDITION_LIMIT and not C.is_exact(profile):
                continue
        break
    else:
        raise AssertionError("{} {}: still ill-conditioned after {} draws".format(case, profile, C.MAX_DRAWS))
    with_values = value_dev is not None and (wanted[1] or wanted[2])
    out = kernels.particle_summary(lw_dev, value_dev if with_values else None, *wanted)
    form = _assert_summary_form(kernels, case, with_values)
    B = case.B
    assert out[0] is None or out[0].shape == (B,)
    for t in out[1:]:
        assert t is None or t.shape == (B,) + case.tail
    errs = _summary_errors([_host(t) for t in out], lw, value if with_values else None)
    assert set(errs) == {name for name, on in zip(("log_ess", "mean", "second"), wanted) if on and (name == "log_ess" or with_values)}
    _hold("K7", case, dtype, profile, form, errs, refs, _summary_bounds(lw), draw + 1)
    return out


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.SUMMARY_CASES, ids=repr)
def test_particle_summary_every_form(kernels, hip_device, case, dtype):
    value, value_dev = _summary_value(case, dtype, hip_device)
    names = C.profile_names(case.K)
    every = (True, value is not None, value is not None)
    full = {name: _check_summary(kernels, hip_device, case, dtype, name, value, value_dev, every) for name in names}
    if value is None:
        return
    # the subsets of outputs that change the launch, on the profile under which most particles count
    name = names[0] if case.K <= C.FLAT_MAX_PARTICLES else "probes"
    for wanted in [(False, True, False), (False, False, True), (True, True, False), (True, False, False), (True, False, True),
                   (False, True, True)]:
        out = _check_summary(kernels, hip_device, case, dtype, name, value, value_dev, wanted)
        for got, whole, on in zip(out[1:], full[name][1:], wanted[1:]):
            assert (got is None) == (not on)
            assert got is None or torch.equal(got, whole)          # the same sums in the same order, whoever else is written


@pytest.mark.parametrize("rest", [R.REST, -np.inf], ids=["rest-1e4", "rest-inf"])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.ONE_HOT_SUMMARY_CASES, ids=repr)
def test_particle_summary_one_hot_at_every_position(kernels, hip_device, case, dtype, rest):
    """Every particle position is the lone weighted particle of some row of some launch (the rows of a launch take
    consecutive positions): mean, second moment and log_ess are exact.  A wrong address, a skipped tail or a slice
    boundary off by one cannot pass."""
    value, value_dev = _summary_value(case, dtype, hip_device)
    B, K = case.B, case.K
    rows = torch.arange(B, device=hip_device)
    level = (0.5 + rows).to(TORCH[dtype])
    bad = torch.zeros((), dtype=torch.int64, device=hip_device)
    seen = torch.zeros(K, dtype=torch.bool, device=hip_device)
    for start in range(0, K, B):
        spots = torch.clamp(start + rows, max=K - 1)
        lw = torch.full((B, K), rest, dtype=TORCH[dtype], device=hip_device)
        lw[rows, spots] = level
        log_ess, mean, second = kernels.particle_summary(lw, value_dev, True, True, True)
        _assert_summary_form(kernels, case)
        want = value_dev[rows, spots]
        bad += (mean != want).sum() + (second != want * want).sum() + (log_ess != 0).sum()
        seen[spots] = True
    assert bool(seen.all())
    assert int(bad) == 0, "{} outputs of the one-hot sweep are not exact".format(int(bad))
    _figures("K7/one_hot_sweep", case, dtype, "one_hot" if rest == R.REST else "one_hot_inf", "S{}".format(case.S), 0.0, 0.0, 0.0)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.SPECIAL_SUMMARY_CASES, ids=repr)
def test_particle_summary_special_slices(kernels, hip_device, case, dtype):
    """NaN, +inf, a slice of -inf, a row of -inf, every second particle -inf — each in the first, a middle and the last
    slice of row 1: the other rows come out bit for bit as without it, the row itself as the convention says (NaN where
    its weights cannot be normalised; the contract's numbers where they can)."""
    value, value_dev = _summary_value(case, dtype, hip_device)
    assert case.S >= 3
    clean = C.weights("flat", case.B, case.K, dtype, C.case_seed(case, "flat"))
    base = kernels.particle_summary(_dev(clean, hip_device), value_dev, True, True, True)
    form = _assert_summary_form(kernels, case)
    others = [b for b in range(case.B) if b != 1]
    for kind in C.SPECIALS:
        for s in (0, 1, case.S - 1):
            lw = np.array(clean, copy=True)
            lw[1] = C.special_row(clean[1], kind, s, case.L)
            lw_dev = _dev(lw, hip_device)
            out = kernels.particle_summary(lw_dev, value_dev, True, True, True)
            _assert_summary_form(kernels, case)
            for got, before in zip(out, base):
                assert torch.equal(got[others], before[others]), "{} {} in slice {}: the rows beside it moved".format(case, kind, s)
            row = [_host(t[1:2]) for t in out]
            if kind in ("nan", "plus_inf", "minus_inf_row"):
                assert all(np.isnan(t).all() for t in row), "{} {} in slice {}".format(case, kind, s)
                continue
            errs = _summary_errors(row, lw[1:2], value[1:2])
            refs = {}
            if dtype == np.float32:
                refs = _summary_errors([_host(t) for t in _eager_summary(lw_dev[1:2], value_dev[1:2])], lw[1:2], value[1:2])
                assert 8.0 * max(refs.values()) <= C.CONDITION_LIMIT
            _hold("K7/special", case, dtype, "{}@{}".format(kind, s), form, errs, refs, _summary_bounds(lw[1:2]))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.API_SUMMARY_CASES, ids=repr)
def test_statistics_api_gives_the_provider_numbers(kernels, hip_device, case, dtype):
    from aesmc_amd import statistics
    value, value_dev = _summary_value(case, dtype, hip_device)
    if case.tail == (20,):
        value, value_dev = value.reshape(case.B, case.K, 4, 5), value_dev.reshape(case.B, case.K, 4, 5)
    tail = tuple(value.shape[2:])
    lw = C.weights(C.API_PROFILE, case.B, case.K, dtype, 0, L=case.L)
    lw_dev = _dev(lw, hip_device)
    log_ess, mean, second = kernels.particle_summary(lw_dev, value_dev, True, True, True)
    assert _summary_form(kernels)["S"] == case.S and _summary_form(kernels)["kernel"] == case.form["kernel"]
    errs = _summary_errors([_host(log_ess), _host(mean), _host(second)], lw, value)
    assert max(errs.values()) <= 16 * EPS32            # under `probes` every sum has ten equal terms
    ess_only = kernels.particle_summary(lw_dev, None, True)[0]
    got = statistics.log_ess(lw_dev)
    assert got.shape == (case.B,) and torch.equal(got, ess_only)
    assert C.error_floor_one(_host(got), R.particle_summary(lw)[0]) <= 16 * EPS32
    assert torch.equal(statistics.ess(lw_dev), torch.exp(ess_only))
    one = statistics.log_ess(lw_dev[0])
    assert one.shape == () and torch.equal(one, kernels.particle_summary(lw_dev[:1], None, True)[0][0])
    got = statistics.empirical_mean(value_dev, lw_dev)
    assert got.shape == (case.B,) + tail and torch.equal(got, mean)
    got = statistics.empirical_variance(value_dev, lw_dev)
    assert got.shape == (case.B,) + tail and torch.equal(got, second - mean ** 2)


# ---- K1 -------------------------------------------------------------------------------------------------------------------
def _assert_logweight_form(kernels, case):
    form = C.logweight_form(kernels._lib.aesmc_test_last_logweight_form())
    assert form == case.form, "{}: ran (TPR, VEC) = {}, meant {}".format(case, form, case.form)
    return "TPR{}{}".format(form[0], "v" if form[1] else "")


def _lse_refs(dtype, rows_dev, want):
    return {"lse": C.error_floor_one(_host(torch.logsumexp(rows_dev, 1)), want)} if dtype == np.float32 else {}


def _lse_bounds(rows, want):
    with np.errstate(all="ignore"):
        return {"lse_bound": float((R.lse_bound(rows) / np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 1.0)))).max())}


def _all_combinations(number, profile):
    """Every combination of optional operands and outputs runs on a case's first profile (the one under which most
    particles count) and on `one_hot`, where the answers are exact; the other profiles run the full one."""
    return number == 0 or profile == "one_hot"


def _drawn_rows(case, dtype, profile, device, rows_of):
    """Weights of `profile` for a K1 case, drawn again while eager float32's log-sum-exp of the rows `rows_of(lw)` the
    launch reduces is ill-conditioned.  Returns (lw, draws)."""
    for draw in range(C.MAX_DRAWS):
        lw = C.weights(profile, case.B, case.K, dtype, C.case_seed(case, profile, draw), L=case.L, centre=True)
        if dtype == np.float64 or C.is_exact(profile):
            return lw, draw + 1
        rows = rows_of(lw)
        if 8.0 * _lse_refs(dtype, _dev(rows, device), R.row_lse(rows))["lse"] <= C.CONDITION_LIMIT:
            return lw, draw + 1
    raise AssertionError("{} {}: still ill-conditioned after {} draws".format(case, profile, C.MAX_DRAWS))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.LOGWEIGHT_CASES, ids=repr)
def test_logweight_lse_every_form(kernels, hip_device, case, dtype):
    names = C.profile_names(case.K, case.ascending)
    for number, profile in enumerate(names):
        target, draws = _drawn_rows(case, dtype, profile, hip_device, lambda lw: lw)
        for which in (C.TERMS if _all_combinations(number, profile) else C.TERMS[-1:]):
            a, b, c = C.terms(target, which, C.case_seed(case, profile))
            want_lw, want_lse = R.logweight_lse(a, b, c)
            operands = [None if t is None else _dev(t, hip_device, case.shift) for t in (a, b, c)]
            lw, lse = kernels.logweight_lse(*operands)
            form = _assert_logweight_form(kernels, case)
            assert np.array_equal(_host(lw), want_lw, equal_nan=True), "{} {} {}: lw is two IEEE operations".format(case, profile, which)
            errs = {"lse": C.error_floor_one(_host(lse), want_lse)}
            _hold("K1/forward", case, dtype, profile + ":" + which, form, errs, _lse_refs(dtype, _dev(want_lw, hip_device), want_lse),
                  _lse_bounds(want_lw, want_lse), draws)
        # a pure row log-sum-exp writes no lw
        assert kernels.logweight_lse(_dev(target, hip_device, case.shift), want_lw=False)[0] is None


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.LOGWEIGHT_CASES, ids=repr)
def test_logweight_accumulate_every_form(kernels, hip_device, case, dtype):
    for number, profile in enumerate(C.profile_names(case.K, case.ascending)):
        seed = C.case_seed(case, profile)
        target, draws = _drawn_rows(case, dtype, profile, hip_device,
                                    lambda lw: R.logweight_accumulate(lw, None, None, C.running_sum(profile, lw, seed))[1])
        a, b, c = C.terms(target, "a+b-c", seed)
        acc = C.running_sum(profile, target, seed)
        want_lw, want_total, want_lse = R.logweight_accumulate(a, b, c, acc)
        operands = [_dev(t, hip_device, case.shift) for t in (a, b, c, acc)]
        for want_out_lw, want_out_lse in ([(True, True), (False, True), (True, False), (False, False)]
                                          if _all_combinations(number, profile) else [(True, True)]):
            lw, total, lse = kernels.logweight_accumulate(*operands, want_lw=want_out_lw, want_lse=want_out_lse)
            form = _assert_logweight_form(kernels, case)
            assert (lw is None) == (not want_out_lw) and (lse is None) == (not want_out_lse)
            assert lw is None or np.array_equal(_host(lw), want_lw, equal_nan=True)
            assert np.array_equal(_host(total), want_total, equal_nan=True), "{} {}: total = acc + lw is an IEEE addition".format(case, profile)
            if lse is not None:
                errs = {"lse": C.error_floor_one(_host(lse), want_lse)}
                _hold("K1/accumulate", case, dtype, profile, form, errs, _lse_refs(dtype, _dev(want_total, hip_device), want_lse),
                      _lse_bounds(want_total, want_lse), draws)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.LOGWEIGHT_CASES, ids=repr)
def test_logweight_backward_every_particle(kernels, hip_device, case, dtype):
    rng = np.random.RandomState(case.B + case.K)
    grad_lw = rng.randn(case.B, case.K).astype(dtype)
    grad_lse = (rng.randn(case.B) + np.where(rng.rand(case.B) < 0.5, -2.0, 2.0)).astype(dtype)
    for number, profile in enumerate(C.profile_names(case.K, case.ascending)):
        drawn = C.weights(profile, case.B, case.K, dtype, C.case_seed(case, profile), L=case.L, centre=True)
        # lw and lse are DATA to the kernel: both on a grid of 2^-10, so that lw - lse is exact in float32 too
        # (reductions.on_grid: the rounding of that difference is shared by every float32 evaluation and not what is
        # measured).  `flat` also runs as drawn, lse the rounded float64 log-sum-exp: there |lw - lse| stays below 16, the
        # shared rounding below 16 eps32 / 2, and generic operands reach the kernel under this metric too.
        for grid in ((True, False) if profile == "flat" else (True,)):
            lw = R.on_grid(drawn) if grid else drawn
            lse = (R.on_grid(R.row_lse(lw)) if grid else R.row_lse(lw)).astype(dtype)
            if grid:
                with np.errstate(all="ignore"):
                    d = lw.astype(np.float64) - lse.astype(np.float64)[:, None]
                    assert np.array_equal(d, (lw - lse[:, None]).astype(np.float64), equal_nan=True)       # exact in the dtype
            lw_dev, glw_dev = _dev(lw, hip_device, case.shift), _dev(grad_lw, hip_device, case.shift)
            lse_dev, glse_dev = _dev(lse, hip_device), _dev(grad_lse, hip_device)
            # the three combinations on the first profile and on `one_hot`; elsewhere grad_lse alone, under which a particle's
            # softmax term is all there is to its gradient (beside a grad_lw of order 1 the metric's denominator is of order 1)
            for use_lw, use_lse in ([(True, True), (False, True), (True, False)] if _all_combinations(number, profile) else [(False, True)]):
                g, ng = kernels.logweight_lse_backward(lw_dev, lse_dev, glw_dev if use_lw else None, glse_dev if use_lse else None)
                form = _assert_logweight_form(kernels, case)
                glw, glse = (grad_lw if use_lw else None), (grad_lse if use_lse else None)
                want, _ = R.logweight_lse_backward(lw, lse, glw, glse)
                scale = R.backward_scale(lw, lse, glw, glse)
                assert torch.equal(ng, -g)
                errs = {"g": C.error_relative(_host(g), want, scale)}
                refs = {}
                if dtype == np.float32:
                    eager = glse_dev[:, None] * torch.exp(lw_dev - lse_dev[:, None]) if use_lse else torch.zeros_like(lw_dev)
                    eager = eager + glw_dev if use_lw else eager
                    refs = {"g": C.error_relative(_host(eager), want, scale)}
                    assert 8.0 * refs["g"] <= C.CONDITION_LIMIT, "{} {}: nothing is summed here, eager float32 is {:.3e} off".format(
                        case, profile, refs["g"])
                # one_hot is exact where only grad_lse arrives (g[b,p] = grad_lse[b], 0 elsewhere) or only grad_lw; with both
                # the sum at the lone particle rounds, and the case's limit holds it
                bounds = {"g_bound": float(R.backward_bound(lw, lse).max()), "g": "limit" if (use_lw and use_lse) else None}
                label = profile + ("" if grid else "/as-drawn") + ":" + ("lw" if use_lw else "") + ("+lse" if use_lse else "")
                _hold("K1/backward", case, dtype, label, form, errs, refs, bounds)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.SPECIAL_LOGWEIGHT_CASES, ids=repr)
def test_logweight_rows_without_a_finite_lse(kernels, hip_device, case, dtype):
    """What include/aesmc_hip.h says of K1 where lse is not finite, in every form.  Forward: a row of -inf gives -inf, a
    +inf particle +inf, a NaN anywhere NaN (also beside a +inf).  Backward, lse being data: the expression as written —
    lse = -inf gives grad_lse times +inf (NaN where lw = -inf too), lse = +inf gives 0 for lw < +inf and NaN at a +inf
    particle, a NaN lse gives NaN; without grad_lse the term is dropped and g = grad_lw whatever lse holds.  All of it is
    held exactly: the special value itself where the contract's is not finite, exact equality where its size is 0."""
    lw, lse_data = C.special_logweight_rows(case, dtype)
    special, finite = [list(rows) for rows in (C.SPECIAL_LOGWEIGHT_ROWS["special"], C.SPECIAL_LOGWEIGHT_ROWS["finite"])]
    lw_dev = _dev(lw, hip_device)
    _, lse = kernels.logweight_lse(lw_dev, want_lw=False)
    form = _assert_logweight_form(kernels, case)
    want_lse = R.row_lse(lw)
    assert not np.isfinite(want_lse[special]).any() and np.isfinite(want_lse[finite]).all()
    assert C.error_floor_one(_host(lse)[special], want_lse[special]) == 0.0, "{}: lse {} for {}".format(case, _host(lse)[special], want_lse[special])
    _hold("K1/special/forward", case, dtype, "finite-rows-beside", form, {"lse": C.error_floor_one(_host(lse)[finite], want_lse[finite])},
          _lse_refs(dtype, lw_dev[finite], want_lse[finite]), _lse_bounds(lw[finite], want_lse[finite]))
    rng = np.random.RandomState(case.K)
    grad_lw = rng.randn(case.B, case.K).astype(dtype)
    grad_lse = np.array([1.5, -2.0, 0.75, -1.25, 2.5, -0.5], dtype=dtype)
    lse_dev, glw_dev, glse_dev = [_dev(t, hip_device) for t in (lse_data, grad_lw, grad_lse)]
    for use_lw, use_lse in [(False, True), (True, True), (True, False)]:
        g, ng = kernels.logweight_lse_backward(lw_dev, lse_dev, glw_dev if use_lw else None, glse_dev if use_lse else None)
        _assert_logweight_form(kernels, case)
        glw, glse = (grad_lw if use_lw else None), (grad_lse if use_lse else None)
        want, want_neg = R.logweight_lse_backward(lw, lse_data, glw, glse)
        scale = R.backward_scale(lw, lse_data, glw, glse)
        if use_lse:
            assert np.isnan(want[0]).all() and np.isnan(want[2]).all() and np.isinf(want[3]).all() and np.isnan(want[1, case.K // 2])
        else:
            assert np.array_equal(want, grad_lw)
        label = ("lw" if use_lw else "") + ("+lse" if use_lse else "")
        for got, expected in ((g, want), (ng, want_neg)):
            err = C.error_relative(_host(got), expected, scale)
            _figures("K1/special/backward", case, dtype, label, form, 0.0, 0.0, err)
            assert err == 0.0, "{} {} {}: a convention of the backward is missed".format(case, np.dtype(dtype).name, label)


@pytest.mark.parametrize("rest", [R.REST, -np.inf], ids=["rest-1e4", "rest-inf"])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", C.ONE_HOT_LOGWEIGHT_CASES, ids=repr)
def test_logweight_one_hot_at_every_position(kernels, hip_device, case, dtype, rest):
    """lse = the lone particle's value, g = grad_lse there and 0 elsewhere, -g its negative: exact, for every position."""
    B, K = case.B, case.K
    rows = torch.arange(B, device=hip_device)
    level = (0.5 + rows).to(TORCH[dtype])
    grad_lse = torch.tensor([1.5, -2.0, 0.25][:B], dtype=TORCH[dtype], device=hip_device)
    bad = torch.zeros((), dtype=torch.int64, device=hip_device)
    for start in range(0, K, B):
        spots = torch.clamp(start + rows, max=K - 1)
        lw = torch.full((B, K), rest, dtype=TORCH[dtype], device=hip_device)
        lw[rows, spots] = level
        _, lse = kernels.logweight_lse(lw, want_lw=False)
        _assert_logweight_form(kernels, case)
        g, ng = kernels.logweight_lse_backward(lw, lse, None, grad_lse)
        _assert_logweight_form(kernels, case)
        want = torch.zeros_like(lw)
        want[rows, spots] = grad_lse
        bad += (lse != level).sum() + (g != want).sum() + (ng != -want).sum()
    assert int(bad) == 0, "{} outputs of the one-hot sweep are not exact".format(int(bad))
    _figures("K1/one_hot_sweep", case, dtype, "one_hot" if rest == R.REST else "one_hot_inf", "TPR{}".format(case.form[0]), 0.0, 0.0, 0.0)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", C.STEP_SHAPES, ids=lambda s: "{}x{}".format(*s))
@pytest.mark.parametrize("entry", C.STEP_ENTRIES)
def test_fused_step_lse_by_product(kernels, hip_device, entry, shape, dtype):
    """resample_step(..., want_lse=True) returns the row log-sum-exp beside the indices: the same contract, the same limit."""
    from aesmc_amd._kernels import PackedAncestors
    B, K = shape
    case = C.STEP_CASES[C.STEP_SHAPES.index(shape)]
    gen = torch.Generator().manual_seed(B * 7 + K)
    u = torch.rand((B, K) if entry == "stratified" else (B,), dtype=torch.float64, generator=gen).to(hip_device)
    for profile in C.STEP_PROFILES:
        lw = C.weights(profile, B, K, dtype, 0, L=case.L)
        lw_dev = _dev(lw, hip_device)
        out = kernels.resample_step(lw_dev, u, None, want_lse=True, want_child_end=(entry == "ranges"), packed=(entry == "packed"))
        assert out is not None, "the fused step declined {}x{}".format(B, K)
        idx, lse, _ = out
        assert isinstance(idx, PackedAncestors) == (entry == "packed" and kernels.step_packs(B, K, lw_dev))
        want = R.row_lse(lw)
        errs = {"lse": C.error_floor_one(_host(lse), want)}
        _hold("K2/lse/" + entry, case, dtype, profile, "step", errs, _lse_refs(dtype, lw_dev, want), _lse_bounds(lw, want))
