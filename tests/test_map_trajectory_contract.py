"""CPU checks of the MAP trajectory (particle Viterbi): the NumPy contract of aesmc_pairwise_argmax
(aesmc_amd/testing/smoothing.py) against a loop over every (row point, column) pair, its tie rule and its conventions for
special values, the whole recursion against the enumeration of every path, the margins that let the device test demand
identical indices, the ABI's argument checks, and the host logic of `aesmc_amd.smoothing.map_trajectory` / `map_smooth` on
a provider that adds `pairwise_argmax` from the contract to the suite's oracle provider."""
import itertools
import math

import numpy as np
import pytest
import torch
from torch.distributions import Laplace, Normal

from aesmc_amd.testing import smoothing as contract
from tests.oracle_provider import OracleKernels


def _operands(rng, B, R, C, D, dtype=np.float64, vector_scale=True):
    rows, cols = rng.randn(B, R, D).astype(dtype), rng.randn(B, C, D).astype(dtype)
    scale = (0.5 + rng.rand(D if vector_scale else 1)).astype(dtype)
    col_a, col_sub, row_add = (2 * rng.randn(B, C)).astype(dtype), rng.randn(B, C).astype(dtype), rng.randn(B, R).astype(dtype)
    return rows, cols, scale, col_a, col_sub, row_add


def brute_force(rows, cols, scale, col_a, col_sub, row_add):
    """One pair at a time in Python floats (IEEE float64): a true division by the scale, exact sums (fsum), the first of
    the largest scores.  Returns (out, arg, gap): gap is the winner's score minus the runner-up's."""
    B, R, D = rows.shape
    C = cols.shape[1]
    out, arg, gap = np.empty((B, R)), np.empty((B, R), dtype=np.int64), np.empty((B, R))
    for b in range(B):
        for r in range(R):
            s = []
            for c in range(C):
                q = math.fsum(((float(rows[b, r, d]) - float(cols[b, c, d])) / float(scale[d if len(scale) > 1 else 0])) ** 2
                              for d in range(D))
                term = float(col_a[b, c]) - (0.0 if col_sub is None else float(col_sub[b, c]))
                s.append(term - 0.5 * q)
            top = max(s)
            arg[b, r] = s.index(top)
            out[b, r] = (0.0 if row_add is None else float(row_add[b, r])) + top
            gap[b, r] = top - max([v for c, v in enumerate(s) if c != arg[b, r]], default=-math.inf)
    return out, arg, gap


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B,R,C,D,vector_scale", [(1, 1, 1, 1, False), (2, 4, 5, 2, True), (2, 7, 33, 3, False),
                                                  (1, 3, 70, 1, True), (2, 5, 9, 0, True)])
def test_contract_equals_a_loop_over_every_pair(dtype, B, R, C, D, vector_scale):
    rng = np.random.RandomState(B * 1000 + C)
    rows, cols, scale, col_a, col_sub, row_add = _operands(rng, B, R, C, D, dtype, vector_scale)
    for sub, add in ((col_sub, row_add), (None, None), (col_sub, None), (None, row_add)):
        out, arg, flags = contract.pairwise_argmax(rows, cols, scale, col_a, sub, add)
        bound = contract.pairwise_argmax_bound(rows, cols, scale, col_a, sub, add)
        assert flags == 0 and out.dtype == np.float64 and arg.dtype == np.int64 and out.shape == arg.shape == bound.shape == (B, R)
        assert (bound > 0).all() and (bound < 1e-12).all()
        want, want_arg, gap = brute_force(rows, cols, scale, col_a, sub, add)
        assert (gap > 2 * bound).all(), (gap.min(), bound.max())          # nothing is excused: every winner is clear
        assert (np.abs(out - want) <= bound).all(), (np.abs(out - want).max(), bound.min())
        assert np.array_equal(arg, want_arg)
        mine = contract.pairwise_argmax_gap(rows, cols, scale, col_a, sub)
        assert np.array_equal(np.isinf(mine), np.isinf(gap)) and (mine > 0).all()
        both = np.isfinite(gap)
        assert (np.abs(mine[both] - gap[both]) <= 2 * bound[both]).all()


def test_ties_go_to_the_smallest_column():
    rng = np.random.RandomState(3)
    B, R, C, D = 2, 5, 40, 3
    rows, cols, scale, col_a, col_sub, row_add = _operands(rng, B, R, C, D)
    col_a[:, 17] += 50.0                                             # column 17 wins everywhere ...
    for twin in (3, 29, 39):                                         # ... and has an exact twin before or after it
        c2, a2 = cols.copy(), col_a.copy()
        c2[:, twin], a2[:, twin] = cols[:, 17], col_a[:, 17]
        s2 = col_sub.copy()
        s2[:, twin] = col_sub[:, 17]
        out, arg, flags = contract.pairwise_argmax(rows, c2, scale, a2, s2, row_add)
        assert flags == 0 and (arg == min(17, twin)).all()
        assert np.array_equal(out, contract.pairwise_argmax(rows, cols, scale, col_a, col_sub, row_add)[0])
        assert (contract.pairwise_argmax_gap(rows, c2, scale, a2, s2) == 0).all()
    same = np.broadcast_to(cols[:, :1], cols.shape)                  # every column identical, equal col_a
    out, arg, _ = contract.pairwise_argmax(rows, same, scale, np.zeros((B, C)))
    assert (arg == 0).all()
    out, arg, _ = contract.pairwise_argmax(rows[:, :, :0], cols[:, :, :0], None, np.full((B, C), 1.5))
    assert (arg == 0).all() and (out == 1.5).all()


def test_special_values():
    rng = np.random.RandomState(1)
    B, R, C, D = 3, 4, 6, 2
    rows, cols, scale, col_a, col_sub, row_add = _operands(rng, B, R, C, D)
    clean, clean_arg, flags = contract.pairwise_argmax(rows, cols, scale, col_a, col_sub, row_add)
    assert flags == 0 and np.isfinite(clean).all() and (clean_arg < C).all()
    nan_flag, degenerate = contract.FLAG_NAN_LOG_WEIGHT, contract.FLAG_DEGENERATE_ROW

    def run(**changed):
        operands = dict(rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add)
        for name, edits in changed.items():
            operands[name] = operands[name].copy()
            for index, value in (edits if isinstance(edits, list) else [edits]):
                operands[name][index] = value
        return contract.pairwise_argmax(**operands), contract.pairwise_argmax_bound(**operands)

    def others_untouched(out, arg, bad):
        assert np.array_equal(out[~bad], clean[~bad]) and np.array_equal(arg[~bad], clean_arg[~bad])

    point = np.zeros((B, R), dtype=bool)
    point[1, 2] = True
    row = np.zeros((B, R), dtype=bool)
    row[1] = True
    # NaN: in a row point, in its row_add (that point alone), in a column or its weights (the whole batch row)
    for changed, bad in ((dict(rows=((1, 2, 0), np.nan)), point), (dict(row_add=((1, 2), np.nan)), point),
                         (dict(cols=((1, 3, 1), np.nan)), row), (dict(col_a=((1, 3), np.nan)), row),
                         (dict(col_sub=((1, 3), np.nan)), row), (dict(scale=(0, np.nan)), np.ones((B, R), dtype=bool))):
        (out, arg, flags), bound = run(**changed)
        assert flags == nan_flag, changed
        assert np.isnan(out[bad]).all() and (arg[bad] == C).all() and (bound[bad] == 0).all()
        others_untouched(out, arg, bad)
    # a largest score of +inf: the flag, out +inf, no column
    for changed in (dict(col_sub=((1, 3), -np.inf)), dict(col_a=((1, 3), np.inf))):
        (out, arg, flags), bound = run(**changed)
        assert flags == degenerate and (out[row] == np.inf).all() and (arg[row] == C).all() and (bound[row] == 0).all()
        others_untouched(out, arg, row)
    # NaN wins over +inf in one row point; different points with each raise both flags
    (out, arg, flags), _ = run(col_a=[((1, 3), np.inf), ((1, 4), np.nan)])
    assert flags == nan_flag and np.isnan(out[row]).all() and (arg[row] == C).all()
    others_untouched(out, arg, row)
    (out, arg, flags), _ = run(col_a=((1, 3), np.inf), row_add=((1, 2), np.nan))
    assert flags == nan_flag | degenerate and np.isnan(out[1, 2]) and (out[1, [0, 1, 3]] == np.inf).all() and (arg[row] == C).all()
    others_untouched(out, arg, row)
    (out, arg, flags), _ = run(col_a=((0, 1), np.inf), rows=((2, 1, 0), np.nan))
    assert flags == nan_flag | degenerate and (out[0] == np.inf).all() and np.isnan(out[2, 1])
    bad = np.zeros((B, R), dtype=bool)
    bad[0], bad[2, 1] = True, True
    others_untouched(out, arg, bad)
    # every score -inf: out -inf, no column and no flag — every column absent, or the one row point infinitely far from all
    (out, arg, flags), bound = run(col_a=((1, slice(None)), -np.inf), col_sub=((1, 0), np.nan))
    assert flags == 0 and (out[row] == -np.inf).all() and (arg[row] == C).all() and (bound[row] == 0).all()
    others_untouched(out, arg, row)
    (out, arg, flags), _ = run(rows=((1, 2, 0), np.inf))
    assert flags == 0 and (out[point] == -np.inf).all() and (arg[point] == C).all()
    others_untouched(out, arg, point)
    # an absent column stays absent whatever col_sub holds, and is never the argument
    (out, arg, flags), _ = run(col_a=((1, int(clean_arg[1, 0])), -np.inf), col_sub=((1, int(clean_arg[1, 0])), -np.inf))
    assert flags == 0 and np.isfinite(out).all() and arg[1, 0] != clean_arg[1, 0] and (arg < C).all()
    # a finite maximum under an infinite row_add keeps its column: the sum is what it is
    (out, arg, flags), bound = run(row_add=((1, 2), -np.inf))
    assert flags == 0 and out[1, 2] == -np.inf and arg[1, 2] == clean_arg[1, 2] and bound[1, 2] == 0
    others_untouched(out, arg, point)


def _log_normal(value, loc, scale):
    return (-0.5 * ((value - loc) / scale) ** 2 - np.log(scale) - 0.5 * np.log(2 * np.pi)).sum(-1)


def _bootstrap_filter(seed, T, B, K, d, dtype=np.float64):
    """A NumPy bootstrap filter on a random linear-Gaussian model.  Returns (x T x [B,K,d], initial_log_prob [B,K],
    emission_log_probs T x [B,K], A, scale [d]): stored particles as a filter leaves them, not a designed input."""
    rng = np.random.RandomState(seed)
    A = 0.9 * np.eye(d) + 0.05 * rng.randn(d, d)
    scale, emission_scale = 0.6 + 0.8 * rng.rand(d), 0.5
    truth = rng.randn(B, d)
    x, emission_log_probs = [], []
    particles = rng.randn(B, K, d)
    initial_log_prob = None
    for t in range(T):
        if t > 0:
            truth = truth @ A.T + scale * rng.randn(B, d)
            log_w = emission_log_probs[-1]
            w = np.exp(log_w - log_w.max(axis=1, keepdims=True))
            ancestors = np.stack([rng.choice(K, size=K, p=w[b] / w[b].sum()) for b in range(B)])
            particles = np.stack([x[-1][b][ancestors[b]] for b in range(B)]) @ A.T + scale * rng.randn(B, K, d)
        y = truth + emission_scale * rng.randn(B, d)
        particles = particles.astype(dtype)
        x.append(particles)
        if t == 0:
            initial_log_prob = _log_normal(particles.astype(np.float64), 0.0, np.ones(d)).astype(dtype)
        emission_log_probs.append(_log_normal(y[:, None, :], particles.astype(np.float64), np.full(d, emission_scale)).astype(dtype))
    return x, initial_log_prob, emission_log_probs, A, scale.astype(dtype)


def test_viterbi_pass_equals_the_enumeration_of_every_path():
    T, B, K, d = 5, 2, 4, 2
    x, initial_log_prob, emission_log_probs, A, scale = _bootstrap_filter(5, T, B, K, d)
    indices, log_joint, (tolerance, margin) = contract.viterbi_pass(x, initial_log_prob, emission_log_probs,
                                                                    lambda t: x[t] @ A.T, scale, return_tolerance=True)
    assert len(indices) == T and all(i.shape == (B,) and i.dtype == np.int64 for i in indices) and log_joint.shape == (B,)
    for b in range(B):
        best, best_path, second = -np.inf, None, -np.inf
        for path in itertools.product(range(K), repeat=T):          # all K^T = 1024 of them
            joint = initial_log_prob[b, path[0]] + sum(emission_log_probs[t][b, path[t]] for t in range(T))
            joint += sum(_log_normal(x[t][b, path[t]], x[t - 1][b, path[t - 1]] @ A.T, scale) for t in range(1, T))
            if joint > best:
                best, best_path, second = joint, path, best
            elif joint > second:
                second = joint
        assert tuple(int(i[b]) for i in indices) == best_path
        assert abs(log_joint[b] - best) <= tolerance[-1][b].max() + 1e-13 * abs(best)      # (the enumeration's own T sums)
        # the margin is a bound from below on how far the second-best PATH lies behind
        assert 0 < margin[b] <= best - second + 1e-12
    assert all((t > 0).all() and t.max() < 1e-12 for t in tolerance)
    # steps with different numbers of particles, one value for the scale, a single step
    ragged = [x[0], x[1][:, :3], x[2], x[3][:, :1], x[4][:, :2]]
    logs = [emission_log_probs[0], emission_log_probs[1][:, :3], emission_log_probs[2], emission_log_probs[3][:, :1],
            emission_log_probs[4][:, :2]]
    indices, log_joint = contract.viterbi_pass(ragged, initial_log_prob, logs, lambda t: ragged[t] @ A.T, scale[:1])
    assert (indices[3] == 0).all() and (indices[1] < 3).all() and (indices[4] < 2).all() and np.isfinite(log_joint).all()
    indices, log_joint = contract.viterbi_pass(x[:1], initial_log_prob, emission_log_probs[:1], None, scale)
    assert np.array_equal(indices[0], (initial_log_prob + emission_log_probs[0]).argmax(axis=1))
    assert np.array_equal(log_joint, (initial_log_prob + emission_log_probs[0]).max(axis=1))
    # a row without any path of positive density: "no column" all the way back, nothing dereferenced
    dead = [e.copy() for e in emission_log_probs]
    dead[2][1] = -np.inf
    indices, log_joint, (_, margin) = contract.viterbi_pass(x, initial_log_prob, dead, lambda t: x[t] @ A.T, scale,
                                                            return_tolerance=True)
    assert log_joint[1] == -np.inf and all(i[1] == K for i in indices) and np.isnan(margin[1]) and np.isfinite(log_joint[0])


def test_margins_on_random_problems_leave_the_path_to_no_rounding():
    """Over 24 seeds of a bootstrap-filtered d = 3, K = 257, T = 6 problem the smallest gap between winner and runner-up
    along the best path stays above 1e-6 — three orders of magnitude above 1e-9, which in turn bounds the recursion's
    float64 tolerance (T (D + 4) eps |delta| = 6 * 7 * 2e-16 * 100 = 1e-12) a thousandfold: what lets the device test
    demand identical indices.  (The issue's own NumPy check over 24 seeds read 3.3e-4.)"""
    smallest, largest_tolerance = np.inf, 0.0
    for seed in range(24):
        x, initial_log_prob, emission_log_probs, A, scale = _bootstrap_filter(100 + seed, 6, 1, 257, 3, np.float32)
        locations = [(x[t].astype(np.float64) @ A.T).astype(np.float32) for t in range(5)]
        _, log_joint, (tolerance, margin) = contract.viterbi_pass(x, initial_log_prob, emission_log_probs,
                                                                  lambda t: locations[t], scale, return_tolerance=True)
        assert np.isfinite(log_joint).all()
        smallest = min(smallest, margin.min())
        largest_tolerance = max(largest_tolerance, max(t.max() for t in tolerance))
    print("\n[viterbi margins] smallest margin along a best path {:.3e}, largest tolerance {:.3e}".format(
        smallest, largest_tolerance))
    assert smallest > 1e-6 and largest_tolerance < 1e-9


def test_the_contract_alone_excuses_no_row_point_of_the_device_tests_inputs():
    """tests/test_gpu_map_trajectory.py demands the contract's `arg` wherever the contract's own gap exceeds twice its
    bound, and excuses at most one row point in 1000 otherwise: on its float32 and float64 inputs the gap exceeds twice
    the bound at EVERY row point of every case that is not tied by construction."""
    from tests import test_gpu_map_trajectory as device
    for dtype in (np.float32, np.float64):
        for shape in device.SHAPES:
            for profile, tied, operands in device.cases(shape, dtype):
                gap = contract.pairwise_argmax_gap(*operands[:5])
                bound = contract.pairwise_argmax_bound(*operands)
                if tied:
                    assert (gap == 0).all() or (gap > 2 * bound).all(), (shape, profile)
                else:
                    assert (gap > 2 * bound).all(), (shape, profile, gap.min(), bound.max())


def test_the_abi_rejects_bad_arguments_before_any_launch():
    """aesmc_pairwise_lse's checks in its order with its statuses; `arg` is optional — no GPU needed."""
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from aesmc_amd import _lib
    lib = _lib.load()
    view = _lib.View3(16, 4, 1, 1)
    ref = ctypes.byref(view)

    def call(rows=ref, cols=ref, scale=16, scale_stride=0, col_a=16, col_sub=None, row_add=None, out=16, arg=16, B=1, R=2, C=4,
             D=1, dtype=0):
        return lib.aesmc_pairwise_argmax(dtype, rows, cols, scale, scale_stride, col_a, col_sub, row_add, out, arg, None, B, R,
                                         C, D, None)

    assert call(col_a=None) == 1 and call(out=None) == 1
    assert call(rows=None) == 1 and call(cols=None) == 1 and call(scale=None) == 1
    assert call(rows=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1 and call(cols=ctypes.byref(_lib.View3(None, 4, 1, 1))) == 1
    assert call(B=-1) == 1 and call(R=-1) == 1 and call(C=-1) == 1 and call(D=-1) == 1
    assert call(dtype=7) == 1 and call(dtype=-1) == 1 and call(scale_stride=2) == 1 and call(scale_stride=-1) == 1
    assert call(C=0) == 1                                            # row points and nothing to maximise over
    assert call(D=257) == 2 and call(R=1 << 30) == 2 and call(C=1 << 31) == 2 and call(B=1 << 31) == 2
    assert call(B=1 << 29, R=64) == 2                                # more workgroups than a grid holds
    assert call(B=0) == 0 and call(R=0) == 0 and call(B=0, D=257) == 0 and call(R=0, C=0) == 0
    assert call(rows=None, cols=None, scale=None, D=0, B=0) == 0     # the D == 0 form takes NULL terms
    assert call(B=0, arg=None) == 0                                  # arg is optional: the maximum only
    assert call(D=257, col_a=None) == 1 and call(D=257, out=None) == 1      # invalid is reported before unsupported
    assert lib.aesmc_version() == 501                                # additive: the ABI's version stays


# ---- the host logic on the oracle provider -----------------------------------------------------------------------------
class ViterbiOracle(OracleKernels):
    """The suite's oracle provider plus `pairwise_argmax` from the NumPy contract, rounded to the operands' dtype."""

    def __init__(self):
        super().__init__()
        self.calls = []

    @staticmethod
    def pairwise_argmax_covers(*operands):
        from aesmc_amd import _kernels
        return _kernels.HipKernels.pairwise_argmax_covers(*operands)

    def pairwise_argmax(self, rows, cols, scale, col_a, col_sub=None, row_add=None):
        if not self.pairwise_argmax_covers(rows, cols, scale, col_a, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_argmax does not take these operands (see pairwise_argmax_covers)")
        n = lambda t: None if t is None else t.detach().numpy()
        self.calls.append(dict(rows=rows, cols=cols, scale=scale, col_a=col_a, col_sub=col_sub, row_add=row_add))
        out, arg, flags = contract.pairwise_argmax(n(rows), n(cols), n(scale), n(col_a), n(col_sub), n(row_add))
        self._flags |= flags
        return torch.from_numpy(out).to(col_a.dtype), torch.from_numpy(arg)


@pytest.fixture
def viterbi_backend():
    from aesmc_amd import _kernels
    provider = ViterbiOracle()
    previous = _kernels._swap_provider_for_tests(provider)
    try:
        yield provider
    finally:
        _kernels._swap_provider_for_tests(previous)


def _filtered(dtype=torch.float64, T=5, B=3, K=24, d=2, affine=False):
    from aesmc_amd import _lazy, inference
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(d, dtype=dtype, affine=affine).tune_proposal()
    observations = model.simulate(T, B, seed=1)
    torch.manual_seed(2)
    np.random.seed(2)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, K,
                          return_latents=True, return_original_latents=True, return_log_weights=True)
    return model, observations, [_lazy.real(x).detach() for x in out["original_latents"]], out["latents"]


def _numpy_viterbi(model, observations, latents, transition=None, emission=None):
    """`viterbi_pass` fed the densities as `state.log_prob` forms them and the locations as the transition gives them."""
    from aesmc_amd import state
    transition, emission = transition or model.transition, emission or model.emission
    T = len(latents)
    with torch.no_grad():
        initial_log_prob = state.log_prob(model.initial(), latents[0]).numpy()
        emission_log_probs = []
        for t in range(T):
            keywords = {} if t == 0 else dict(previous_observations=observations[:t])
            distribution = emission(latents=latents[:t + 1], time=t, **keywords)
            emission_log_probs.append(state.log_prob(
                distribution, state.expand_observation(observations[t], latents[t].shape[1])).numpy())
        locations = [transition(previous_latents=latents[:t + 1], time=t + 1, previous_observations=observations[:t + 1])
                     .loc.numpy() for t in range(T - 1)]
    return contract.viterbi_pass([x.numpy() for x in latents], initial_log_prob, emission_log_probs, lambda t: locations[t],
                                 np.array([float(model.transition_scale)]), return_tolerance=True)


def _last_place(values, dtype):
    return np.spacing(np.abs(values).astype(np.float32)).astype(np.float64) if dtype == torch.float32 else 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_map_trajectory_equals_the_numpy_viterbi_pass(viterbi_backend, dtype):
    from aesmc_amd import smoothing
    model, observations, latents, _ = _filtered(dtype)
    T, (B, K, d) = len(latents), latents[0].shape
    seen = []

    def initial():
        seen.append(("initial",))
        return model.initial()

    def transition(previous_latents=None, time=None, previous_observations=None):
        assert all(type(x) is torch.Tensor and not x.requires_grad for x in previous_latents)
        seen.append(("transition", time, len(previous_latents), len(previous_observations),
                     all(a.data_ptr() == b.data_ptr() for a, b in zip(previous_latents, latents)),
                     torch.equal(previous_observations[-1], observations[time - 1])))
        return model.transition(previous_latents=previous_latents, time=time, previous_observations=previous_observations)

    def emission(latents=None, time=None, **keywords):
        assert all(type(x) is torch.Tensor and not x.requires_grad for x in latents)
        seen.append(("emission", time, len(latents), tuple(keywords), len(keywords.get("previous_observations", ()))))
        return model.emission(latents=latents, time=time, **keywords)

    stored = [x.clone() for x in latents]
    trajectory, log_joint, indices = smoothing.map_trajectory(latents, initial, transition, emission, observations,
                                                              return_indices=True)
    # each callable once per step, forwards in time, with exactly the arguments `infer` and the other smoothers hand over
    want_calls = [("initial",), ("emission", 0, 1, (), 0)]
    for t in range(1, T):
        want_calls += [("transition", t, t, t, True, True), ("emission", t, t + 1, ("previous_observations",), t)]
    assert seen == want_calls
    want, want_joint, (tolerance, margin) = _numpy_viterbi(model, observations, latents)
    largest = max(t.max() for t in tolerance)
    assert (margin > 2 * largest).all(), (margin, largest)           # the path is decided by no rounding
    assert len(trajectory) == len(indices) == T and log_joint.shape == (B,) and log_joint.dtype == dtype
    for t in range(T):
        assert indices[t].dtype == torch.int64 and np.array_equal(indices[t].numpy(), want[t]), t
        assert trajectory[t].shape == (B, d) and trajectory[t].dtype == dtype and not trajectory[t].requires_grad
        assert torch.equal(trajectory[t], stored[t][torch.arange(B), indices[t]])          # the stored values, bit for bit
        assert torch.equal(latents[t], stored[t])                                            # ... which are left alone
    error = np.abs(log_joint.numpy().astype(np.float64) - want_joint)
    assert (error <= tolerance[-1].max(axis=1) + _last_place(want_joint, dtype)).all(), (error, tolerance[-1].max())
    # T - 1 launches in float64 whatever the latents' dtype, then the final maximum without a distance term
    calls = viterbi_backend.calls
    assert len(calls) == T
    for t in range(1, T):
        call = calls[t - 1]
        assert all(call[name].dtype == torch.float64 for name in ("rows", "cols", "scale", "col_a", "row_add"))
        assert torch.equal(call["rows"], latents[t].double()) and call["col_sub"] is None and call["cols"].shape == (B, K, d)
    assert calls[-1]["rows"].shape == (B, 1, 0) and calls[-1]["cols"].shape == (B, K, 0) and calls[-1]["scale"] is None
    assert calls[-1]["col_sub"] is None and calls[-1]["row_add"] is None and calls[-1]["col_a"].dtype == torch.float64
    pair, joint_again = smoothing.map_trajectory(latents, model.initial, model.transition, model.emission, observations)
    assert all(torch.equal(a, b) for a, b in zip(pair, trajectory)) and torch.equal(joint_again, log_joint)


def test_log_joint_is_at_least_that_of_every_genealogy_path(viterbi_backend):
    from aesmc_amd import smoothing
    for dtype, slack in ((torch.float64, 1e-9), (torch.float32, 1e-4)):      # (float32 densities: T (2 d + 1) terms of 1e-6)
        model, observations, latents, genealogy = _filtered(dtype, T=6, K=40)
        _, log_joint = smoothing.map_trajectory(latents, model.initial, model.transition, model.emission, observations)
        A, C = model.A.detach().double().numpy(), model.C.detach().double().numpy()
        sx, sy = float(model.transition_scale), float(model.emission_scale)
        paths = [x.detach().double().numpy() for x in genealogy]             # T x [B,K,d]: path k is paths[:][b,k]
        y = [o.double().numpy() for o in observations]
        joint = _log_normal(paths[0], 0.0, np.ones(2))
        for t in range(len(paths)):
            joint = joint + _log_normal(y[t][:, None, :], paths[t] @ C.T, np.full(2, sy))
            if t > 0:
                joint = joint + _log_normal(paths[t], paths[t - 1] @ A.T, np.full(2, sx))
        assert (log_joint.double().numpy() >= joint.max(axis=1) - slack).all(), (log_joint, joint.max(axis=1))


def test_one_step_steps_of_different_size_and_an_emission_that_is_not_normal(viterbi_backend):
    from aesmc_amd import smoothing, state
    model, observations, latents, _ = _filtered()
    B = latents[0].shape[0]
    # T = 1: the initial and emission densities, the final maximum and no distance launch
    trajectory, log_joint, indices = smoothing.map_trajectory(latents[:1], model.initial, model.transition, model.emission,
                                                              observations[:1], return_indices=True)
    want, want_joint, _ = _numpy_viterbi(model, observations[:1], latents[:1])
    assert len(viterbi_backend.calls) == 1 and viterbi_backend.calls[0]["rows"].shape == (B, 1, 0)
    assert np.array_equal(indices[0].numpy(), want[0]) and np.array_equal(log_joint.numpy(), want_joint)
    assert torch.equal(trajectory[0], latents[0][torch.arange(B), indices[0]])
    # steps that hold different numbers of particles
    ragged = [latents[0], latents[1][:, :7], latents[2], latents[3][:, :1], latents[4][:, :13]]
    trajectory, log_joint, indices = smoothing.map_trajectory(ragged, model.initial, model.transition, model.emission,
                                                              observations, return_indices=True)
    want, want_joint, (tolerance, _) = _numpy_viterbi(model, observations, ragged)
    assert all(np.array_equal(i.numpy(), w) for i, w in zip(indices, want)) and (indices[3] == 0).all()
    assert (np.abs(log_joint.numpy() - want_joint) <= tolerance[-1].max(axis=1)).all()
    assert all(torch.equal(trajectory[t], ragged[t][torch.arange(B), indices[t]]) for t in range(5))
    # a Laplace emission: anything `state.log_prob` takes
    full = state.BatchShapeMode.FULLY_EXPANDED

    def emission(latents=None, time=None, previous_observations=None):
        return state.set_batch_shape_mode(Laplace(latents[-1] @ model.C.t(), 0.7), full)

    _, log_joint, indices = smoothing.map_trajectory(latents, model.initial, model.transition, emission, observations,
                                                     return_indices=True)
    want, want_joint, (tolerance, margin) = _numpy_viterbi(model, observations, latents, emission=emission)
    assert (margin > 2 * max(t.max() for t in tolerance)).all()
    assert all(np.array_equal(i.numpy(), w) for i, w in zip(indices, want))
    assert (np.abs(log_joint.numpy() - want_joint) <= tolerance[-1].max(axis=1)).all()
    gauss, _ = _numpy_viterbi(model, observations, latents)[:2]
    assert any(not np.array_equal(a, b) for a, b in zip(gauss, want))          # ... and it is not the Normal's answer


def test_it_is_deterministic_and_leaves_the_random_states_alone(viterbi_backend):
    from aesmc_amd import distributed, smoothing
    model, observations, latents, _ = _filtered()
    np.random.seed(11)
    torch.manual_seed(3)
    numpy_before, torch_before = np.random.get_state(), torch.get_rng_state()
    first, joint = smoothing.map_trajectory(latents, model.initial, model.transition, model.emission, observations)
    numpy_after = np.random.get_state()
    assert numpy_before[0] == numpy_after[0] and (numpy_before[1] == numpy_after[1]).all() and \
        numpy_before[2:] == numpy_after[2:]
    assert torch.equal(torch_before, torch.get_rng_state())
    with distributed.shard_scope(2 * latents[0].shape[0], 0, 2):      # rows are independent: nothing to refuse
        sharded, sharded_joint = smoothing.map_trajectory(latents, model.initial, model.transition, model.emission,
                                                          observations)
    assert all(torch.equal(a, b) for a, b in zip(first, sharded)) and torch.equal(joint, sharded_joint)


def test_refusals(viterbi_backend):
    from aesmc_amd import smoothing, state
    full = state.BatchShapeMode.FULLY_EXPANDED
    model, observations, latents, _ = _filtered()
    T, (B, K, d) = len(latents), latents[0].shape
    tag = lambda dist, mode=full: state.set_batch_shape_mode(dist, mode)
    loc = lambda previous_latents: previous_latents[-1] @ model.A.t()
    run = lambda transition: smoothing.map_trajectory(latents, model.initial, transition, model.emission, observations)
    with pytest.raises(NotImplementedError, match="dict latents"):
        smoothing.map_trajectory([{"x": x} for x in latents], model.initial, model.transition, model.emission, observations)
    with pytest.raises(NotImplementedError, match="Laplace"):
        run(lambda previous_latents=None, **kw: tag(Laplace(loc(previous_latents), 1.0)))
    with pytest.raises(NotImplementedError, match="particle-dependent"):
        run(lambda previous_latents=None, **kw: tag(Normal(loc(previous_latents), torch.ones(B, K, d, dtype=torch.float64))))
    with pytest.raises(NotImplementedError, match="FULLY_EXPANDED"):
        run(lambda previous_latents=None, **kw: tag(Normal(torch.zeros(d, dtype=torch.float64), 1.0),
                                                    state.BatchShapeMode.NOT_EXPANDED))
    wide = [torch.zeros(2, 3, 257, dtype=torch.float64) for _ in range(2)]
    with pytest.raises(NotImplementedError, match="D > 256"):
        smoothing.map_trajectory(
            wide, lambda: tag(Normal(torch.zeros(257, dtype=torch.float64), 1.0), state.BatchShapeMode.NOT_EXPANDED),
            lambda previous_latents=None, **kw: tag(Normal(previous_latents[-1], 1.0)),
            lambda latents=None, **kw: tag(Normal(latents[-1], 1.0)), [torch.zeros(2, 257, dtype=torch.float64)] * 2)
    with pytest.raises(ValueError, match="equally long"):
        smoothing.map_trajectory(latents, model.initial, model.transition, model.emission, observations[:-1])
    with pytest.raises(ValueError, match="not empty"):
        smoothing.map_trajectory([], model.initial, model.transition, model.emission, [])
    assert viterbi_backend.read_flags(None) == 0


class _Spiked(Normal):
    """A Normal whose log-density is overwritten at chosen places: densities a model can hand over and no Normal has."""

    def __init__(self, loc, scale, edits):
        super().__init__(loc, scale)
        self.edits = edits

    def log_prob(self, value):
        out = super().log_prob(value).clone()
        for index, held in self.edits:
            out[index] = held
        return out


def test_bad_rows_are_raised_once_at_the_end(viterbi_backend):
    from aesmc_amd import smoothing, state
    model, observations, latents, _ = _filtered()
    T = len(latents)
    run = lambda x=latents, emission=model.emission: smoothing.map_trajectory(x, model.initial, model.transition, emission,
                                                                              observations)

    def spiked_emission(at, edits):
        def emission(latents=None, time=None, previous_observations=None):
            dist = model.emission(latents=latents, time=time, previous_observations=previous_observations)
            if time != at:
                return dist
            return state.set_batch_shape_mode(_Spiked(dist.loc, dist.scale, edits), state.BatchShapeMode.FULLY_EXPANDED)
        return emission

    poisoned = spiked_emission(1, [((0, 3), float("nan"))])          # a NaN density at one particle of one step
    with pytest.raises(FloatingPointError):
        run(emission=poisoned)
    assert len(viterbi_backend.calls) == T                      # every step ran: the flags are read once, at the end
    assert viterbi_backend.read_flags(None) == 0                # ... and are left clear
    del viterbi_backend.calls[:]
    with pytest.raises(RuntimeError, match="no finite maximum"):          # a density of +inf: a degenerate row point
        run(emission=spiked_emission(1, [((2, 5), float("inf"))]))
    assert len(viterbi_backend.calls) == T and viterbi_backend.read_flags(None) == 0
    del viterbi_backend.calls[:]
    with pytest.raises(RuntimeError, match="no path of positive density.*\\[1\\]"):      # a batch row of all -inf
        run(emission=spiked_emission(2, [((1,), -float("inf"))]))
    assert len(viterbi_backend.calls) == T and viterbi_backend.read_flags(None) == 0
    # an exception in a callable leaves nothing behind either
    def broken(latents=None, time=None, previous_observations=None):
        if time == 3:
            raise KeyError("mine")
        return poisoned(latents=latents, time=time, previous_observations=previous_observations)
    with pytest.raises(KeyError):
        run(emission=broken)
    assert viterbi_backend.read_flags(None) == 0
    # single particles of zero density are no error: the path avoids them
    trajectory, log_joint, indices = smoothing.map_trajectory(
        latents, model.initial, model.transition, spiked_emission(2, [((1, slice(0, 5)), -float("inf"))]), observations,
        return_indices=True)
    assert torch.isfinite(log_joint).all() and indices[2][1] >= 5


def test_map_smooth_is_infer_followed_by_map_trajectory(viterbi_backend):
    from aesmc_amd import inference, smoothing
    from aesmc_amd.testing.models import LgssmNd
    model = LgssmNd(2, dtype=torch.float64).tune_proposal()
    observations = model.simulate(4, 3, seed=1)
    torch.manual_seed(9)
    np.random.seed(9)
    trajectory, log_joint, log_z = smoothing.map_smooth(observations, model.initial, model.transition, model.emission,
                                                        model.proposal, 16)
    torch.manual_seed(9)
    np.random.seed(9)
    out = inference.infer("smc", observations, model.initial, model.transition, model.emission, model.proposal, 16,
                          return_log_marginal_likelihood=True, return_latents=False, return_original_latents=True,
                          return_log_weight=False, return_log_weights=True)
    want, want_joint = smoothing.map_trajectory(out["original_latents"], model.initial, model.transition, model.emission,
                                                observations)
    assert torch.equal(log_z, out["log_marginal_likelihood"]) and torch.equal(log_joint, want_joint)
    assert len(trajectory) == 4 and all(torch.equal(a, b) for a, b in zip(trajectory, want))
    assert trajectory[0].shape == (3, 2) and log_joint.shape == (3,)
