"""CPU checks of the status codes of the switching-model entries of include/aesmc_hip.h: what each of the sixteen refuses
(status 1), what it does not support (status 2), what it takes as an empty launch (status 0), and the order of the three.

No test here can launch a kernel on its made-up pointers: every status-1 case has B = 0 or K = 0 (validation precedes the
empty-launch return, so a check that went missing gives 0, not a launch), and the cases that need sizes run only without
a GPU, where a call that passes every check ends in AESMC_ERR_LAUNCH."""
import ctypes

import pytest
import torch

from aesmc_amd import _lib

ERR_LAUNCH = 3          # every check passed; without a device the launch then fails
LIMIT = 0x7fffffff
TRI = 8 * 9 // 2            # packed elements of a covariance at the largest D
OPERANDS = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="non-empty sizes on made-up pointers: only where nothing can launch")


class Entry:
    """One C entry with a valid set of made-up arguments: `order` names them as the entry takes them, every pointer a
    distinct multiple of 64, `model` a dict of SwitchingModel fields or None."""

    def __init__(self, name, order, absent=(), **sizes):
        self.name, self.order = name, order
        self.valid = {arg: 64 * (i + 1) for i, arg in enumerate(order)}
        self.valid.update({arg: None for arg in absent})
        self.valid.update(stream=None, **sizes)
        if "model" in order:
            self.valid["model"] = dict({key: 8 * (i + 1) for i, key in enumerate(OPERANDS)}, M=2, D=2, Dy=1)

    def __call__(self, fields=None, **changes):
        """The status with `changes` to the valid arguments; `fields`: changes to the model's fields."""
        args = dict(self.valid, **changes)
        if args.get("model") is not None:
            args["model"] = ctypes.byref(_lib.SwitchingModel(**dict(args["model"], **(fields or {}))))
        return getattr(_lib.load(), "aesmc_switching_" + self.name)(*[args[arg] for arg in self.order])

    def later(self, **changes):
        """A later step: the three stored operands given (the entries' step 0 passes none of them)."""
        stored = {arg: 4096 + 64 * i for i, arg in enumerate(self.stored)}
        return self(**dict(stored, **changes))


def _kalman(name, *extra):
    head = ("y_dtype", "model", "regime_in", "mean_in", "cov_in", "idx", "uniforms")
    tail = ("regime_out", "mean_out", "cov_out", "log_weight", "flags", "B", "K", "stream")
    order = head + tuple(e for e in extra if e != "observed") + ("y",) + tuple(e for e in extra if e == "observed") + tail
    entry = Entry(name, order, absent=("regime_in", "mean_in", "cov_in", "idx"), y_dtype=_lib.F64, B=0, K=3)
    entry.stored = ("regime_in", "mean_in", "cov_in")
    return entry


def _lookahead(name, outputs, *extra):
    order = ("y_dtype", "model", "log_prior", "regime_in", "mean_in", "cov_in", "y") + extra + outputs + \
        ("flags", "B", "K", "stream")
    entry = Entry(name, order, absent=("regime_in", "mean_in", "cov_in"), y_dtype=_lib.F64, B=0, K=3)
    entry.stored = ("regime_in", "mean_in", "cov_in")
    return entry


def _information(name, *extra):
    order = ("y_dtype", "model", "regime_next", "omega_in", "lambda_in", "c_in", "y") + extra + \
        ("omega_out", "lambda_out", "c_out", "factor_out", "flags", "B", "K", "stream")
    entry = Entry(name, order, absent=("omega_in", "lambda_in", "c_in"), y_dtype=_lib.F64, B=0, K=3)
    entry.stored = ("omega_in", "lambda_in", "c_in")
    return entry


def _smooth(name, *extra):
    order = ("model", "regime_next", "mean", "cov", "factor", "lambda", "omega_next", "cov_next") + extra + \
        ("mean_out", "cov_out", "cross_out", "flags", "B", "K", "D", "stream")
    return Entry(name, order, B=0, K=3, D=2)


KALMAN = [_kalman("kalman_step"), _kalman("kalman_draw", "particle_cdf"), _kalman("kalman_conditional_step", "pinned_regime"),
          _kalman("kalman_masked_step", "particle_cdf", "pinned_regime", "observed")]
LOOKAHEAD = [_lookahead("lookahead", ("log_weight", "cdf")), _lookahead("masked_lookahead", ("log_weight", "cdf"), "observed"),
             _lookahead("lookahead_scores", ("cdf", "log_weight")),
             _lookahead("masked_lookahead_scores", ("cdf", "log_weight"), "observed")]
INFORMATION = [_information("information_step"), _information("masked_information_step", "observed")]
SMOOTH = [_smooth("smooth_combine"), _smooth("masked_smooth_combine", "observed")]
WITH_Y = KALMAN + LOOKAHEAD + INFORMATION
BACKWARD = Entry("backward_scores", ("log_Pi", "regime_next", "factor", "lambda", "regime", "mean", "cov", "log_w", "scores",
                                     "flags", "B", "K", "N", "M", "D", "stream"), B=0, K=3, N=2, M=2, D=2)
CONDITIONAL = Entry("conditional_ancestor_index", ("log_w", "u", "log_Pi", "regime_next", "factor", "lambda", "regime", "mean",
                                                   "cov", "idx", "flags", "B", "K", "M", "D", "stream"), B=0, K=3, M=2, D=2)
RESAMPLE = Entry("optimal_resample", ("log_w", "scores", "u", "parent", "regime", "log_weight", "lse", "count", "flags", "B",
                                      "K", "M", "K_out", "stream"), B=0, K=3, M=2, K_out=4)
INT32 = ("regime_in", "regime_next", "regime_out", "regime", "pinned_regime", "flags", "count")      # 4-byte operands
BYTES = ("observed",)

ids = dict(ids=lambda entry: entry.name)


def _pointers(entry):
    return [arg for arg in entry.order if arg not in ("y_dtype", "model", "B", "K", "N", "M", "D", "K_out", "stream")]


def _misaligned(arg):
    return 2 if arg in INT32 else 4


@pytest.mark.parametrize("entry", WITH_Y + SMOOTH + [BACKWARD, CONDITIONAL, RESAMPLE], **ids)
def test_empty_launches_are_taken(entry):
    assert entry() == 0
    assert entry(B=2, K=0) == 0
    if hasattr(entry, "stored"):
        assert entry.later() == 0 and entry.later(B=2, K=0) == 0
    assert entry(B=-1) == 1 and entry(K=-1) == 1


def test_limit_getters():
    lib = _lib.load()
    assert (lib.aesmc_switching_max_latent_dim(), lib.aesmc_switching_max_observation_dim(),
            lib.aesmc_switching_max_regimes()) == (8, 8, 16)
    assert [lib.aesmc_switching_conditional_max_particles(D) for D in range(-1, 11)] == \
        [0, 0] + [8192] * 4 + [4096] * 4 + [0, 0]
    assert lib.aesmc_switching_optimal_resample_max_candidates() == 16384


@pytest.mark.parametrize("entry", WITH_Y, **ids)
def test_model_and_observation_checks(entry):
    info = entry in INFORMATION
    assert entry(model=None) == 1
    for field in ("M", "D", "Dy"):
        assert entry(fields={field: 0}) == 1
    for key in OPERANDS[2:]:
        unread = info and key in ("m0", "s0")      # K34 does not read the initial state
        assert entry(fields={key: None}) == (0 if unread else 1), key
        assert entry(fields={key: 4}) == (0 if unread else 1), key
        assert entry.later(fields={key: None}) == (0 if unread else 1), key
    # the chain's rows: only K31 and K38 read them, cdf0 at step 0 and cdf later; K39 reads them unless particle_cdf is given (as it is here)
    reads_rows = entry.name in ("kalman_step", "kalman_conditional_step")
    assert entry(fields={"cdf0": None}) == entry(fields={"cdf0": 4}) == entry.later(fields={"cdf": None}) == \
        entry.later(fields={"cdf": 4}) == (1 if reads_rows else 0)
    assert entry(fields={"cdf": None}) == entry.later(fields={"cdf0": None}) == 0
    if entry.name == "kalman_masked_step":
        assert entry(fields={"cdf0": None}, pinned_regime=None) == 0          # K33's form
        assert entry(fields={"cdf0": None}, particle_cdf=None) == 1           # K38's
    assert entry(y=None) == 1
    for tag in (-1, 2, 5):
        assert entry(y_dtype=tag) == 1
    assert entry(y=4) == 1 and entry(y=4, y_dtype=_lib.F32) == 0 and entry(y=2, y_dtype=_lib.F32) == 1
    # the stored operands come together
    for given in range(1, 7):
        some = {arg: 4096 + 64 * i for i, arg in enumerate(entry.stored) if given >> i & 1}
        assert entry(**some) == 1, sorted(some)
    # the orderings: an invalid argument beside an unsupported extent is invalid; an unsupported extent of an empty launch is not looked at
    for extent in ({"D": 9}, {"Dy": 9}, {"M": 17}):
        assert entry(fields=extent) == 0 and entry(fields=extent, B=2, K=0) == 0
        assert entry(fields=extent, y=None) == 1 and entry(fields=dict(extent, A=None)) == 1


@pytest.mark.parametrize("entry", WITH_Y + SMOOTH + [BACKWARD, CONDITIONAL, RESAMPLE], **ids)
def test_misaligned_operands(entry):
    given = dict(entry.valid) if not hasattr(entry, "stored") else \
        dict(entry.valid, **{arg: 4096 + 64 * i for i, arg in enumerate(entry.stored)})
    if "idx" in given and entry in KALMAN:
        given["idx"] = 8192
    for arg in _pointers(entry):
        if arg in BYTES or arg == "y":
            continue
        assert entry(**dict(given, **{arg: given[arg] + _misaligned(arg)})) == 1, arg


@pytest.mark.parametrize("entry", KALMAN, **ids)
def test_kalman_step_operands(entry):
    for arg in ("uniforms", "regime_out", "mean_out", "cov_out", "log_weight"):
        assert entry(**{arg: None}) == 1, arg
    assert entry(flags=None) == 0 and entry(idx=8192) == 0      # (an index at step 0 is not read)
    for out, stored in (("regime_out", "regime_in"), ("mean_out", "mean_in"), ("cov_out", "cov_in")):
        assert entry.later(**{stored: entry.valid[out]}) == 1, out
    if entry.name == "kalman_draw":
        assert entry(particle_cdf=None) == 1
    if "particle_cdf" in entry.order:
        for out in ("mean_out", "cov_out", "log_weight"):
            assert entry(particle_cdf=entry.valid[out]) == 1, out
    if entry.name == "kalman_conditional_step":
        assert entry(pinned_regime=None) == 1
    if "pinned_regime" in entry.order:
        assert entry(pinned_regime=entry.valid["regime_out"]) == 1
    if entry.name == "kalman_masked_step":
        assert entry(observed=None) == 1
        assert entry(particle_cdf=None) == entry(pinned_regime=None) == entry(particle_cdf=None, pinned_regime=None) == 0
        assert entry(observed=entry.valid["observed"] + 1) == 0      # bytes: no alignment
        for out in ("regime_out", "mean_out", "cov_out", "log_weight"):
            assert entry(observed=entry.valid[out]) == 1, out


@pytest.mark.parametrize("entry", LOOKAHEAD, **ids)
def test_lookahead_operands(entry):
    for arg in ("log_prior", "log_weight", "cdf"):
        assert entry(**{arg: None}) == 1, arg
    assert entry(flags=None) == 0
    assert entry(cdf=entry.valid["log_weight"]) == 1
    for out in ("log_weight", "cdf"):
        for stored in ("mean_in", "cov_in"):
            assert entry.later(**{stored: entry.valid[out]}) == 1, (out, stored)
    if "observed" in entry.order:
        assert entry(observed=None) == 1 and entry(observed=entry.valid["observed"] + 1) == 0
        for out in ("log_weight", "cdf"):
            assert entry(observed=entry.valid[out]) == 1, out


@pytest.mark.parametrize("entry", INFORMATION, **ids)
def test_information_operands(entry):
    outputs = ("omega_out", "lambda_out", "c_out", "factor_out")
    for arg in ("regime_next",) + outputs:
        assert entry(**{arg: None}) == 1, arg
    assert entry(flags=None) == 0
    for i, out in enumerate(outputs):
        for source in ("regime_next", "y") + outputs[:i]:
            assert entry(**{out: entry.valid[source]}) == 1, (out, source)
        for stored in entry.stored:
            assert entry.later(**{stored: entry.valid[out]}) == 1, (out, stored)
    if "observed" in entry.order:
        assert entry(observed=None) == 1 and entry(observed=entry.valid["observed"] + 1) == 0
        for out in outputs:
            assert entry(observed=entry.valid[out]) == 1, out


@pytest.mark.parametrize("entry", SMOOTH, **ids)
def test_smooth_combine_operands(entry):
    masked = "observed" in entry.order
    for arg in ("mean", "cov", "factor", "lambda", "mean_out", "cov_out"):
        assert entry(**{arg: None}) == 1, arg
    assert entry(D=0) == 1 and entry(flags=None) == 0 and entry(omega_next=None) == 0
    # with cross_out: the model, regime_next and cov_next are read
    for arg in ("model", "regime_next", "cov_next"):
        assert entry(**{arg: None}) == 1, arg
    assert entry(fields={"M": 0}) == 1 and entry(fields={"Dy": 0}) == 1 and entry(fields={"D": 3}) == 1
    for key in OPERANDS[4:]:
        assert entry(fields={key: None}) == 1 and entry(fields={key: 4}) == 1, key
    for key in OPERANDS[:4]:      # K36 reads neither the chain's rows nor the initial state
        assert entry(fields={key: None}) == 0 and entry(fields={key: 4}) == 0, key
    # without cross_out: what only the cross-covariance reads must not be given; the masked entry needs cross_out
    nothing = dict(cross_out=None, model=None, regime_next=None, omega_next=None, cov_next=None)
    assert entry(**nothing) == (1 if masked else 0)
    assert entry(**dict(nothing, B=2, K=0)) == (1 if masked else 0)
    for arg in ("model", "regime_next", "omega_next", "cov_next"):
        assert entry(**dict(nothing, **{arg: entry.valid[arg]})) == 1, arg
    outputs = ("mean_out", "cov_out", "cross_out")
    inputs = ("regime_next", "mean", "cov", "factor", "lambda", "omega_next", "cov_next")
    for i, out in enumerate(outputs):
        for source in inputs + outputs[:i]:
            assert entry(**{out: entry.valid[source]}) == 1, (out, source)
    if not masked:
        assert entry(**dict(nothing, cov_out=entry.valid["mean"])) == 1 and entry(**dict(nothing, cov_out=entry.valid["mean_out"])) == 1
    if masked:
        assert entry(observed=None) == 1 and entry(observed=entry.valid["observed"] + 1) == 0
        for out in outputs:
            assert entry(observed=entry.valid[out]) == 1, out
    # the orderings
    for extent in ({"D": 9}, {"Dy": 9}, {"M": 17}):
        size = {"D": 9} if "D" in extent else {}
        assert entry(fields=extent, **size) == 0
        assert entry(fields=extent, mean=None, **size) == 1 and entry(fields=dict(extent, A=None), **size) == 1
    if not masked:
        assert entry(**dict(nothing, D=9)) == 0 and entry(**dict(nothing, D=9, mean=None)) == 1


def test_backward_scores_operands():
    entry = BACKWARD
    for arg in _pointers(entry):
        assert entry(**{arg: None}) == (0 if arg in ("log_w", "flags") else 1), arg
    assert entry(N=-1) == 1 and entry(M=0) == 1 and entry(D=0) == 1
    assert entry(B=2, N=0) == 0 and entry(B=2, K=0) == 0
    for arg in ("log_Pi", "regime_next", "factor", "lambda", "regime", "mean", "cov", "log_w"):
        assert entry(scores=entry.valid[arg]) == 1, arg
    assert entry(D=9) == 0 and entry(M=17) == 0 and entry(D=9, mean=None) == 1 and entry(M=17, scores=4) == 1


def test_conditional_ancestor_index_operands():
    entry = CONDITIONAL
    for arg in ("log_w", "u", "idx"):
        assert entry(**{arg: None}) == 1, arg
    assert entry(M=0) == 1 and entry(D=0) == 1 and entry(flags=None) == 0
    assert entry(factor=None) == 1 and entry(**{"lambda": None}) == 1      # the two come together
    plain = dict(factor=None, **{"lambda": None})
    assert entry(**plain) == 0
    for arg in ("log_Pi", "regime_next", "regime", "mean", "cov"):      # read only with the factor
        assert entry(**{arg: None}) == 1, arg
        assert entry(**dict(plain, **{arg: None})) == 0, arg
    for arg in ("log_w", "u", "log_Pi", "regime_next", "factor", "lambda", "regime", "mean", "cov"):
        assert entry(idx=entry.valid[arg]) == 1, arg
    assert entry(D=9) == 0 and entry(M=17) == 0 and entry(D=9, u=None) == 1 and entry(K=1 << 20) == 0


def test_optimal_resample_operands():
    entry = RESAMPLE
    for arg in _pointers(entry):
        assert entry(**{arg: None}) == (0 if arg in ("log_w", "flags") else 1), arg
    assert entry(M=0) == 1 and entry(K_out=-1) == 1
    assert entry(B=2, K=0) == 0 and entry(B=2, K_out=0) == 0
    outputs = ("parent", "regime", "log_weight", "lse", "count")
    for i, out in enumerate(outputs):
        for other in ("log_w", "scores", "u", "flags") + outputs[:i]:
            assert entry(**{out: entry.valid[other]}) == 1, (out, other)
    assert entry(M=17) == 0 and entry(M=17, u=None) == 1


# ---- status 2: sizes are needed, so these run only where nothing can launch ---------------------------------------------------

@no_gpu
@pytest.mark.parametrize("entry", WITH_Y, **ids)
def test_unsupported_extents_and_sizes(entry):
    for call in (entry, entry.later):
        for extent in ({"D": 9}, {"Dy": 9}, {"M": 17}):
            assert call(fields=extent, B=2) == 2, extent
        assert call(B=LIMIT + 1, K=1) == 2 and call(B=1, K=LIMIT + 1) == 2
        assert call(B=1, K=LIMIT // TRI + 1) == 2 and call(B=1 << 16, K=1 << 16) == 2
    assert entry(B=1, K=LIMIT // TRI) == ERR_LAUNCH        # the bound itself passes every check


@no_gpu
@pytest.mark.parametrize("entry", SMOOTH, **ids)
def test_smooth_combine_unsupported(entry):
    assert entry(fields={"D": 9}, D=9, B=2) == 2 and entry(fields={"Dy": 9}, B=2) == 2 and entry(fields={"M": 17}, B=2) == 2
    assert entry(B=LIMIT + 1, K=1) == 2 and entry(B=1, K=LIMIT + 1) == 2
    assert entry(B=1, K=LIMIT // 64 + 1) == 2        # D * D elements per row, not D (D + 1) / 2
    assert entry(B=1, K=LIMIT // 64) == ERR_LAUNCH
    if "observed" not in entry.order:
        nothing = dict(cross_out=None, model=None, regime_next=None, omega_next=None, cov_next=None)
        assert entry(**dict(nothing, D=9, B=2)) == 2 and entry(**dict(nothing, B=1, K=LIMIT // 64 + 1)) == 2


@no_gpu
def test_backward_and_conditional_and_resample_unsupported():
    entry = BACKWARD
    assert entry(D=9, B=2) == 2 and entry(M=17, B=2) == 2
    assert entry(B=LIMIT + 1) == 2 and entry(B=1, K=LIMIT + 1) == 2 and entry(B=1, N=LIMIT + 1) == 2
    assert entry(B=1, K=LIMIT // TRI + 1, N=1) == 2 and entry(B=1, K=1, N=LIMIT // TRI + 1) == 2
    assert entry(B=1, K=1 << 16, N=1 << 16) == 2        # B N K scores
    assert entry(B=1, K=LIMIT // TRI, N=1) == ERR_LAUNCH
    entry = CONDITIONAL
    lib = _lib.load()
    assert entry(D=9, B=2) == 2 and entry(M=17, B=2) == 2 and entry(B=LIMIT + 1) == 2
    for D in (2, 4, 5, 8):
        most = lib.aesmc_switching_conditional_max_particles(D)
        assert entry(D=D, B=1, K=most + 1) == 2, D
    assert entry(D=2, B=1, K=8192) == ERR_LAUNCH
    assert entry(B=LIMIT // TRI // 64 + 1, K=64) == 2 and entry(B=LIMIT // TRI // 64, K=64) == ERR_LAUNCH
    entry = RESAMPLE
    assert entry(M=17, B=2) == 2 and entry(B=1, K=16385, M=1) == 2 and entry(B=1, K=8193, M=2) == 2
    assert entry(B=LIMIT + 1) == 2 and entry(B=1, K_out=LIMIT + 1) == 2 and entry(B=1 << 16, K_out=1 << 16) == 2
    assert entry(B=1, K=8192, M=2) == ERR_LAUNCH
