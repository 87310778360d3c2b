"""CPU checks of aesmc_amd/testing/reductions.py, the float64 contract the K1 / K7 tests hold the kernels to:

  * it is what torch computes in float64 (logsumexp, softmax-weighted sums, the gradient expression) and what
    oracle/kernel_oracle.py says on the inputs of the older tests in tests/test_gpu_kernels.py;
  * the special rows follow include/aesmc_hip.h;
  * the profiles keep their promises (ESS of `flat`, exact zeros of `probes`, exact answers of `one_hot`, no gradient
    whose size sits in the dtype's subnormal range);
  * THE INPUTS HAVE TEETH: for every (profile, shape) pair the GPU module runs, the contract evaluated with one counted
    particle left out, one counted twice, or one slice left out moves at least one output by >= 1e-4 under the GPU
    module's metric — ten times the conditioning cap that bounds the limit a case can be given.  A condition on the
    inputs: no kernel runs here.
"""
import numpy as np
import pytest
import torch

from aesmc_amd.testing import reductions as R
from oracle import kernel_oracle
from tests import reduction_cases as C


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ---- the contract is the operation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_logweight_contract_is_torch_float64(dtype):
    rng = np.random.RandomState(1)
    for shape in [(1, 1), (3, 7), (4, 1000), (2, 4100)]:
        a, b, c, acc = [(3 * rng.randn(*shape)).astype(dtype) for _ in range(4)]
        lw, lse = R.logweight_lse(a, b, c)
        assert lw.dtype == dtype and np.array_equal(lw, ((_t(a) + _t(b)) - _t(c)).numpy())
        want = torch.logsumexp(_t(lw).double(), dim=1).numpy()
        assert np.abs(lse - want).max() <= R.lse_bound(lw).max()
        old_lw, old_lse = kernel_oracle.logweight_lse(a, b, c)
        assert np.array_equal(old_lw, lw)
        np.testing.assert_allclose(old_lse, lse, rtol=4 * np.finfo(dtype).eps, atol=4 * np.finfo(dtype).eps)
        lw2, total, lse2 = R.logweight_accumulate(a, b, c, acc)
        assert np.array_equal(lw2, lw) and np.array_equal(total, (_t(acc) + _t(lw)).numpy())
        assert np.array_equal(total, kernel_oracle.logweight_accumulate(a, b, c, acc)[1])
        assert np.abs(lse2 - torch.logsumexp(_t(total).double(), dim=1).numpy()).max() <= R.lse_bound(total).max()
        for use_lw, use_lse in [(True, True), (False, True), (True, False)]:
            glw = rng.randn(*shape) if use_lw else None
            glse = rng.randn(shape[0]) if use_lse else None
            g, ng = R.logweight_lse_backward(lw, lse, glw, glse)
            x = _t(lw).double().requires_grad_()
            out = torch.logsumexp(x, dim=1)
            loss = (out * _t(glse)).sum() if use_lse else out.sum() * 0
            if use_lw:
                loss = loss + (x * _t(glw)).sum()
            loss.backward()
            scale = R.backward_scale(lw, lse, glw, glse)
            assert C.error_relative(x.grad.numpy(), g, scale) <= 4 * R.backward_bound(lw, lse).max() + 1e-13
            assert np.array_equal(ng, -g)
            old = kernel_oracle.logweight_lse_backward(lw.astype(np.float64), lse, glw, glse)[0]
            np.testing.assert_allclose(old, g, rtol=1e-14, atol=1e-14)


def test_summary_contract_is_torch_float64_and_the_oracle():
    rng = np.random.RandomState(2)
    for (B, K, tail), scale in [((4, 1000, (10,)), 1.0), ((3, 5, (2, 3)), 8.0), ((2, 257, (18,)), 8.0), ((2, 16, ()), 1.0)]:
        lw = rng.randn(B, K) * scale
        value = rng.randn(B, K, *tail)
        log_ess, mean, second = R.particle_summary(lw, value)
        w = torch.softmax(_t(lw), dim=1).reshape((B, K) + (1,) * len(tail))
        first_size, second_size = R.summary_magnitudes(lw, value)
        assert C.error_relative((w * _t(value)).sum(1).numpy(), mean, first_size) <= R.summary_bound(lw).max()
        assert C.error_relative((w * _t(value) ** 2).sum(1).numpy(), second, second_size) <= R.summary_bound(lw).max()
        want = (2 * torch.logsumexp(_t(lw), 1) - torch.logsumexp(2 * _t(lw), 1)).numpy()
        assert np.abs(log_ess - want).max() <= R.log_ess_bound(lw).max() + 4 * R.EPSILON * np.abs(lw).max()
    assert kernel_oracle.particle_summary.__doc__ and "reductions" in kernel_oracle.particle_summary.__doc__      # one definition
    assert R.particle_summary(rng.randn(2, 5))[1:] == (None, None)


def test_special_rows_follow_the_header():
    a = np.random.RandomState(3).randn(6, 40)
    a[0, :] = -np.inf
    a[1, 5] = np.inf
    a[2, 7] = np.nan
    a[2, 9] = np.inf                  # NaN wins over +inf
    a[3, 3:30] = -np.inf
    a[4] += 1e6
    lse = R.row_lse(a)
    assert lse[0] == -np.inf and lse[1] == np.inf and np.isnan(lse[2]) and np.isfinite(lse[3:]).all()
    assert np.array_equal(np.isnan(lse), np.isnan(torch.logsumexp(_t(a), 1).numpy()))
    assert (R.lse_bound(a)[:3] == 0).all() and (R.lse_bound(a)[3:] > 0).all()
    assert R.row_lse(np.zeros((2, 0))).tolist() == [-np.inf, -np.inf]
    # backward with lse as data, evaluated as written
    g, _ = R.logweight_lse_backward(a, lse, None, np.ones(6))
    assert np.isnan(g[0]).all()                                           # -inf - (-inf)
    assert np.isnan(g[1, 5]) and (np.delete(g[1], 5) == 0).all()          # +inf - +inf; finite - inf
    assert np.isnan(g[2]).all()
    assert (g[3, 3:30] == 0).all() and abs(g[3].sum() - 1) < 1e-12
    glw = np.ones((6, 40))
    assert np.array_equal(R.logweight_lse_backward(a, lse, glw, None)[0], glw)        # the term is dropped, not 0 * NaN
    assert (R.backward_bound(a, lse)[0] == 0).all() and (R.backward_bound(a, lse)[3, 3:30] == 0).all()
    # K7: NaN, +inf and all -inf rows give NaN; -inf particles and offsets are fine
    value = R.values(6, 40, (3,))
    log_ess, mean, second = R.particle_summary(a, value)
    assert np.isnan(log_ess[:3]).all() and np.isnan(mean[:3]).all() and np.isnan(second[:3]).all()
    assert np.isfinite(log_ess[3:]).all() and np.isfinite(mean[3:]).all()
    assert (R.log_ess_bound(a)[:3] == 0).all() and (R.summary_bound(a)[:3] == 0).all()
    assert abs(log_ess[4] - R.particle_summary(a[4:5] - 1e6)[0][0]) < 1e-9
    assert (R.summary_magnitudes(a, value)[0][:3] == 0).all()


# ---- the profiles' promises ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_profiles_keep_their_promises(dtype):
    B, K, L = 3, 1537, 513
    for name in ("flat", "minus_inf_stretch", "offset_up", "offset_down"):
        lw = C.weights(name, B, K, dtype, 5)
        assert lw.dtype == dtype
        live = np.isfinite(lw).sum(axis=1)
        assert (R.effective_sample_size(lw) >= live / 4.0).all(), name
    R.assert_flat(C.weights("flat", B, K, dtype, 5))
    with pytest.raises(AssertionError):
        R.assert_flat(C.weights("wide", B, K, dtype, 5))
    shift = 1e6 if dtype == np.float64 else 1e4
    assert abs(C.weights("offset_up", B, K, dtype, 5).mean() - shift) < 1 and abs(C.weights("offset_down", B, K, dtype, 5).mean() + shift) < 1
    lw = C.weights("dominant", B, K, dtype, 5)
    for b in range(B):
        assert int(np.argmax(lw[b])) == R.dominant_position(b, K) >= K - 1 - K // 4
    up, down = R.ascending(B, K, dtype), R.descending(B, K, dtype)
    assert (np.diff(up.astype(np.float64), axis=1) == 1 / 128.0).all() and np.array_equal(down, up[:, ::-1])
    assert (np.diff(R.ascending(2, 8192, np.float32).astype(np.float64), axis=1) == 1 / 128.0).all()
    # probes: exact zeros elsewhere, weights exactly 1 / n, in the dtype's own arithmetic
    at = R.probe_positions(K, L)
    assert at == [0, 63, 64, 255, 256, 512, 513, 1025, 1026, 1536]
    for rest in (R.REST, -np.inf):
        lw = R.probes(B, K, dtype, L=L, rest=rest)
        e = np.exp(lw - lw.max(axis=1, keepdims=True).astype(dtype))
        assert e.dtype == dtype and (np.delete(e, at, axis=1) == 0).all() and (e[:, at] == 1).all()
        value = R.values(B, K, (5,))
        log_ess, mean, _ = R.particle_summary(lw, value)
        np.testing.assert_allclose(log_ess, np.log(len(at)), rtol=1e-15)
        np.testing.assert_allclose(mean, value[:, at].mean(axis=1), rtol=1e-14)
    # one_hot: every answer exact
    spots = C.one_hot_positions(B, K, L)
    for rest in (R.REST, -np.inf):
        lw = R.one_hot(B, K, dtype, spots, rest=rest)
        value = R.values(B, K, (5,))
        log_ess, mean, second = R.particle_summary(lw, value)
        rows = np.arange(B)
        assert (log_ess == 0).all() and np.array_equal(mean, value[rows, spots]) and np.array_equal(second, value[rows, spots] ** 2)
        lse = R.row_lse(lw)
        assert np.array_equal(lse, 0.5 + rows)
        glse = np.array([1.5, -2.0, 0.25])
        g, _ = R.logweight_lse_backward(lw, lse, None, glse)
        assert np.array_equal(g[rows, spots], glse) and np.count_nonzero(g) == B
    values = R.values(2, 300, (17,))
    assert values.min() >= -125 and values.max() <= 125 and np.array_equal(values, values.astype(np.float32))
    assert len({tuple(row) for row in values[0]}) == 251         # 251 distinct particles before the pattern repeats


# ---- teeth -----------------------------------------------------------------------------------------------------------------
def _summary_outputs(lw, value):
    log_ess, mean, second = R.particle_summary(lw, value)
    return log_ess, mean, second


def _summary_moved(case, lw, value, mutated_lw, mutated_value):
    want = _summary_outputs(lw, value)
    got = _summary_outputs(mutated_lw, mutated_value)
    moved = C.error_floor_one(got[0], want[0])
    if value is not None:
        first, second = R.summary_magnitudes(lw, value)
        moved = max(moved, C.error_relative(got[1], want[1], first), C.error_relative(got[2], want[2], second))
    return moved


def _mutations(lw, L, row):
    k = R.least_counted(lw, row)
    yield "particle {} left out".format(k), lambda v: R.drop_particle(lw, v, row, k)
    yield "particle {} counted twice".format(k), lambda v: R.double_particle(lw, v, row, k)
    s = R.least_counted_slice(lw, L, row)
    yield "slice {} left out".format(s), lambda v: R.drop_slice(lw, v, row, s, L)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.SUMMARY_CASES + C.SPECIAL_SUMMARY_CASES, ids=repr)
def test_summary_inputs_have_teeth(case, dtype):
    _, value = case.value()
    value = None if value is None else value[sorted({0, case.B - 1})]
    names = C.profile_names(case.K) if case in C.SUMMARY_CASES else ("flat",) + ((C.API_PROFILE,) if case in C.API_SUMMARY_CASES else ())
    for name in names:
        rows = sorted({0, case.B - 1})                 # the first and the last row stand for the others
        lw = C.weights(name, case.B, case.K, dtype, C.case_seed(case, name), L=case.L)[rows]
        for row in range(len(rows)):
            assert R.counted(lw)[row].any(), (case, name)
            for what, mutate in _mutations(lw, case.L, row):
                moved = _summary_moved(case, lw, value, *mutate(value))
                assert moved >= C.TEETH, "{} {}: {} moves the outputs by {:.3g} only".format(case, name, what, moved)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.LOGWEIGHT_CASES + C.STEP_CASES, ids=repr)
def test_logweight_inputs_have_teeth(case, dtype):
    rows = sorted({0, case.B - 1})                     # the first and the last row stand for the others
    glse = 1.0 + np.arange(len(rows)) / 8.0
    for name in (C.STEP_PROFILES if case in C.STEP_CASES else C.profile_names(case.K, case.ascending)):
        lw = C.weights(name, case.B, case.K, dtype, C.case_seed(case, name), L=case.L, centre=True)[rows]
        lse = R.row_lse(lw)
        g, _ = R.logweight_lse_backward(lw, lse, None, glse)
        for row in range(len(rows)):
            assert R.counted(lw)[row].any(), (case, name)
            for what, mutate in _mutations(lw, case.L, row):
                acc = C.running_sum(name, lw, C.case_seed(case, name))
                mutated, mutated_acc = mutate(acc)
                with np.errstate(all="ignore"):      # under an offset lse is +-1e6: the particle shows in the total's lse
                    moved = max(C.error_floor_one(R.row_lse(mutated), lse),
                                C.error_floor_one(R.row_lse(mutated_acc + mutated), R.row_lse(acc + lw)))
                assert moved >= C.TEETH, "{} {}: {} moves lse by {:.3g} only".format(case, name, what, moved)
            # the backward: a particle's gradient is measured against its own size, so ANY particle written as 0, as its
            # neighbour's value or twice its own is an error of order 1 — where its own size is not 0
            k = R.least_counted(lw, row)
            scale = R.backward_scale(lw, lse, None, glse)
            wrong = np.array(g, copy=True)
            wrong[row, k] = 0.0
            assert C.error_relative(wrong, g, scale) >= 0.5


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_no_gradient_sits_in_the_subnormal_range(dtype):
    """exp(lw - lse) of a particle is either exactly 0 in `dtype` or a normal number with room: a relative metric without
    a floor is then well defined for every particle (a subnormal would carry few bits)."""
    tiny = float(np.finfo(dtype).tiny)
    for case in C.LOGWEIGHT_CASES:
        for name in C.profile_names(case.K, case.ascending):
            lw = C.weights(name, case.B, case.K, dtype, C.case_seed(case, name), L=case.L, centre=True)
            with np.errstate(all="ignore"):
                d = lw.astype(np.float64) - R.row_lse(lw)[:, None]
            d = d[np.isfinite(d)]
            ok = (d >= np.log(tiny) + 5) | (d <= (-745.2 if dtype == np.float64 else -104.0))
            assert ok.all(), (case, name, d[~ok][:4])


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_the_rows_without_a_finite_lse_are_what_they_say(dtype):
    for case in C.SPECIAL_LOGWEIGHT_CASES:
        lw, lse = C.special_logweight_rows(case, dtype)
        true = R.row_lse(lw)
        assert true[0] == -np.inf and true[1] == np.inf and np.isnan(true[[2, 5]]).all() and np.isfinite(true[[3, 4]]).all()
        assert np.array_equal(true[[0, 1, 2, 5]], lse[[0, 1, 2, 5]].astype(np.float64), equal_nan=True)
        g, _ = R.logweight_lse_backward(lw, lse, None, np.array([1.5, -2.0, 0.75, -1.25, 2.5, -0.5]))
        assert np.isnan(g[0]).all() and np.isnan(g[2]).all() and np.isnan(g[5]).all()
        assert np.isnan(g[1, case.K // 2]) and (np.delete(g[1], case.K // 2) == 0).all()
        assert (g[3] == -np.inf).all() and (g[4] == 0).all()
        assert (R.backward_scale(lw, lse, None, np.ones(6))[4] == 0).all() and (R.backward_bound(lw, lse)[[0, 3, 4]] == 0).all()


def test_the_restated_slicing_and_the_form_words():
    assert [C.slices(*bk) for bk in [(3, 700), (2, 1536), (1, 2100), (3, 5000), (700, 40), (1, 200000), (64, 1100)]] == \
        [1, 3, 4, 9, 1, 256, 2]
    word = 1 | 4 | (3 << 3) | (4 << 12) | (1 << 21)
    assert C.summary_form(word) == {"kernel": 1, "dense": True, "S": 3, "TX": 4, "sweeps": 1}
    assert C.logweight_form(2 * 256 + 1) == (256, True) and C.logweight_form(2 * 64) == (64, False)
    for case in C.SUMMARY_CASES + C.ONE_HOT_SUMMARY_CASES + C.SPECIAL_SUMMARY_CASES:
        assert case.form["S"] == case.S, case
        base, view = case.value()
        if view is not None:
            assert view.shape == (case.B, case.K) + case.tail, case
    for case in C.ONE_HOT_SUMMARY_CASES + C.SPECIAL_SUMMARY_CASES:
        assert case.S >= (3 if case in C.SPECIAL_SUMMARY_CASES else 2)
    largest = max(case.B * case.base_K * int(np.prod(case.base_tail)) * 8 for case in C.SUMMARY_CASES if case.tail is not None)
    assert largest <= 17 * 2 ** 20 and max(c.B * (c.K + c.shift) * 8 for c in C.LOGWEIGHT_CASES) <= 17 * 2 ** 20
