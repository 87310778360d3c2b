"""The shapes, profiles and expected forms that tests/test_gpu_reductions_every_particle.py runs and that
tests/test_reductions_contract.py proves to have teeth: one list, so the two cannot drift.  No GPU, no torch."""
import numpy as np

from aesmc_amd.testing import reductions

DTYPES = (np.float32, np.float64)
FLAT_MAX_PARTICLES = 4200         # 1 / K is the smallest effect of one particle under `flat`: beyond, it sinks below 1e-4
CONDITION_LIMIT = 1e-5            # a float32 case whose 8 e_ref exceeds this is drawn again
TEETH = 1e-4                      # what a mutation has to move: ten times the conditioning cap
MAX_DRAWS = 8

SMALL, GENERAL4, GENERAL16 = 1, 2, 3


# ---- the launchers' records ------------------------------------------------------------------------------------------------
def summary_form(word):
    """aesmc_test_last_particle_summary_form() taken apart: kernel, dense, S, TX (the small kernel: R, particles per lane
    per tile), sweeps (the small kernel: tiles per slice)."""
    return {"kernel": word & 3, "dense": bool(word & 4), "S": (word >> 3) & 511, "TX": (word >> 12) & 511,
            "sweeps": (word >> 21) & 1023}


def logweight_form(word):
    """aesmc_test_last_logweight_form() taken apart: (TPR, VEC)."""
    return word // 2, bool(word % 2)


def slices(B, K):
    """S of particle_summary.hip's pick_slices, restated: min(ceil(1024 / B), K // 512, 256), at least 1."""
    return max(1, min((1024 + B - 1) // B, K // 512, 256))


def slice_length(B, K):
    S = slices(B, K)
    return (K + S - 1) // S


# ---- K7 ----------------------------------------------------------------------------------------------------------------
class SummaryCase:
    """One launch shape of K7.  `view`: how the value operand is cut from a larger base (None: dense) — a function of the
    base array / tensor; `base_tail` the base's trailing shape and `base_K` its particle extent."""

    def __init__(self, name, B, K, tail, form, view=None, base_K=None, base_tail=None):
        self.name, self.B, self.K, self.tail, self.form = name, B, K, tuple(tail) if tail is not None else None, form
        self.view, self.base_K, self.base_tail = view, base_K or K, tuple(base_tail) if base_tail is not None else self.tail

    def value(self):
        """(base float64, its view float64) — None, None for a log_ess-only case."""
        if self.tail is None:
            return None, None
        base = reductions.values(self.B, self.base_K, self.base_tail)
        return base, (base if self.view is None else self.view(base))

    @property
    def S(self):
        return slices(self.B, self.K)

    @property
    def L(self):
        return slice_length(self.B, self.K)

    def __repr__(self):
        return self.name


def _form(kernel, S, dense=False, TX=None, sweeps=None):
    return {key: val for key, val in (("kernel", kernel), ("S", S), ("dense", dense), ("TX", TX), ("sweeps", sweeps))
            if val is not None}


def _every_second(base):
    return base[:, ::2]


def _columns_1_9(base):
    return base[..., 1:9]


def _columns_1_129(base):
    return base[..., 1:129]


SUMMARY_CASES = [
    SummaryCase("small-dense-3x700x3", 3, 700, (3,), _form(SMALL, 1, True, TX=5, sweeps=1)),
    SummaryCase("small-3x701x3", 3, 701, (3,), _form(SMALL, 1, False, TX=5)),
    SummaryCase("small-dense-2x1536x4", 2, 1536, (4,), _form(SMALL, 3, True, TX=4, sweeps=1)),          # slice 512 < tile 1024
    SummaryCase("small-2x1537x5", 2, 1537, (5,), _form(SMALL, 3, False, TX=3)),                         # ragged last slice
    SummaryCase("small-1x2100x16", 1, 2100, (16,), _form(SMALL, 4, None, TX=1, sweeps=3)),              # 525 = 256 + 256 + 13
    SummaryCase("small-strided-k-2x800x6", 2, 800, (6,), _form(SMALL, 1, False, TX=2), _every_second, base_K=1600),
    SummaryCase("small-strided-d-2x1100x8", 2, 1100, (8,), _form(SMALL, 2, False, TX=2), _columns_1_9, base_tail=(11,)),
    SummaryCase("general4-5x300x2", 5, 300, (2,), _form(GENERAL4, 1, TX=2, sweeps=1)),
    SummaryCase("general4-2x1100x1", 2, 1100, (1,), _form(GENERAL4, 2, TX=1, sweeps=1)),
    SummaryCase("general4-2x1100x2", 2, 1100, (2,), _form(GENERAL4, 2, TX=2, sweeps=1)),
    SummaryCase("general4-3x300x17", 3, 300, (17,), _form(GENERAL4, 1, TX=17, sweeps=1)),
    SummaryCase("general4-1x1500x17", 1, 1500, (17,), _form(GENERAL4, 2, TX=17, sweeps=1)),
    SummaryCase("general4-1x40x1030", 1, 40, (1030,), _form(GENERAL4, 1, TX=256, sweeps=2)),
    SummaryCase("general4-1x1024x1030", 1, 1024, (1030,), _form(GENERAL4, 2, TX=256, sweeps=2)),
    SummaryCase("general16-2x300x20", 2, 300, (20,), _form(GENERAL16, 1, TX=5, sweeps=1)),
    SummaryCase("general16-2x1024x128", 2, 1024, (128,), _form(GENERAL16, 2, TX=32, sweeps=1)),
    SummaryCase("general16-1x33x2048", 1, 33, (2048,), _form(GENERAL16, 1, TX=256, sweeps=2)),
    SummaryCase("general16-1x1024x2052", 1, 1024, (2052,), _form(GENERAL16, 2, TX=256, sweeps=3)),
    SummaryCase("general4-misaligned-2x1100x128", 2, 1100, (128,), _form(GENERAL4, 2, TX=128, sweeps=1), _columns_1_129,
                base_tail=(130,)),
    SummaryCase("ess-only-3x5000", 3, 5000, None, _form(GENERAL4, 9, TX=1, sweeps=1)),
    SummaryCase("ess-only-700x40", 700, 40, None, _form(GENERAL4, 1, TX=1, sweeps=1)),
]

# one S > 1 shape per kernel: the one-hot sweep (64 rows a launch take 64 consecutive positions), the special slices
# (S = 3) and the API level
ONE_HOT_SUMMARY_CASES = [
    SummaryCase("small-dense-64x1536x4", 64, 1536, (4,), _form(SMALL, 3, True, TX=4)),
    SummaryCase("small-64x1537x5", 64, 1537, (5,), _form(SMALL, 3, False, TX=3)),
    SummaryCase("general4-64x1100x2", 64, 1100, (2,), _form(GENERAL4, 2, TX=2)),
    SummaryCase("general16-64x1024x20", 64, 1024, (20,), _form(GENERAL16, 2, TX=5)),
]
SPECIAL_SUMMARY_CASES = [
    SummaryCase("small-4x1537x5", 4, 1537, (5,), _form(SMALL, 3, False, TX=3)),
    SummaryCase("small-dense-4x1536x4", 4, 1536, (4,), _form(SMALL, 3, True, TX=4)),
    SummaryCase("general4-4x1600x2", 4, 1600, (2,), _form(GENERAL4, 3, TX=2)),
    SummaryCase("general16-4x1540x20", 4, 1540, (20,), _form(GENERAL16, 3, TX=5)),
]
API_SUMMARY_CASES = [SPECIAL_SUMMARY_CASES[0], SPECIAL_SUMMARY_CASES[2], SPECIAL_SUMMARY_CASES[3]]
API_PROFILE = "probes"
SPECIALS = ("nan", "plus_inf", "minus_inf_slice", "minus_inf_row", "every_second_minus_inf")


def special_row(row, kind, s, L):
    """`row` [K] with the convention `kind` put into slice s (length L)."""
    row = np.array(row, copy=True)
    lo, hi = s * L, min(len(row), (s + 1) * L)
    if kind == "nan":
        row[(lo + hi) // 2] = np.nan
    elif kind == "plus_inf":
        row[(lo + hi) // 2] = np.inf
    elif kind == "minus_inf_slice":
        row[lo:hi] = -np.inf
    elif kind == "minus_inf_row":
        row[:] = -np.inf
    elif kind == "every_second_minus_inf":
        row[(s % 2)::2] = -np.inf
    else:
        raise ValueError(kind)
    return row


# ---- K1 ----------------------------------------------------------------------------------------------------------------
class LogweightCase:
    """(B, K), the form (TPR, VEC) it must report, `shift`: operands start this many elements into a larger buffer."""

    def __init__(self, B, K, tpr, vec, shift=0, ascending=False):
        self.B, self.K, self.form, self.shift, self.ascending = B, K, (tpr, vec), shift, ascending
        self.name = "{}x{}{}".format(B, K, "+{}".format(shift) if shift else "")
        self.L = 64          # the stretch the `slice` mutation leaves out: a wavefront's worth of consecutive particles

    def __repr__(self):
        return self.name


LOGWEIGHT_CASES = [
    LogweightCase(5, 64, 64, True), LogweightCase(7, 252, 64, True),
    LogweightCase(5, 63, 64, False), LogweightCase(6, 255, 64, False, ascending=True),
    LogweightCase(2048, 1024, 64, True), LogweightCase(2050, 1023, 64, False),
    LogweightCase(3, 256, 256, True), LogweightCase(2, 4100, 256, True), LogweightCase(2, 8192, 256, True, ascending=True),
    LogweightCase(3, 257, 256, False), LogweightCase(2, 4099, 256, False, ascending=True),
    LogweightCase(3, 260, 256, False, shift=1), LogweightCase(6, 252, 64, False, shift=1),
]
ONE_HOT_LOGWEIGHT_CASES = [LogweightCase(3, 257, 256, False), LogweightCase(2, 4100, 256, True)]
STEP_SHAPES = [(3, 1025), (2, 4096)]
STEP_ENTRIES = ("plain", "ranges", "packed", "stratified")
STEP_PROFILES = ("probes", "probes_inf", "one_hot", "one_hot_inf")
STEP_CASES = [LogweightCase(B, K, 0, False) for B, K in STEP_SHAPES]          # the fused step records no K1 form
# one shape per form of K1 (and the long vector row) for the rows whose lse is not finite
SPECIAL_LOGWEIGHT_CASES = [LogweightCase(6, 64, 64, True), LogweightCase(6, 63, 64, False), LogweightCase(6, 256, 256, True),
                           LogweightCase(6, 257, 256, False), LogweightCase(6, 4100, 256, True)]
SPECIAL_LOGWEIGHT_ROWS = {"special": (0, 1, 2, 5), "finite": (3, 4)}


def special_logweight_rows(case, dtype):
    """(lw [6,K], lse [6] as DATA for the backward), both of `dtype`: row 0 nothing but -inf (lse -inf); row 1 a +inf
    particle in the middle (lse +inf); row 2 a NaN as the last particle (lse NaN); rows 3 and 4 finite flat rows that the
    backward is handed lse = -inf and lse = +inf for; row 5 a NaN first and a +inf last (lse NaN: NaN wins)."""
    assert case.B == 6
    K = case.K
    lw = reductions.centred(reductions.flat(6, K, dtype, case_seed(case, "special")))
    lw[0, :] = -np.inf
    lw[1, K // 2] = np.inf
    lw[2, K - 1] = np.nan
    lw[5, 0], lw[5, K - 1] = np.nan, np.inf
    lse = np.array([-np.inf, np.inf, np.nan, -np.inf, np.inf, np.nan], dtype=dtype)
    return lw, lse

TERMS = ("a", "a+b", "a-c", "a+b-c")


def terms(lw, which, seed):
    """(a, b, c) of lw's dtype with a + b - c == lw where that is exact: b, c multiples of 1 / 8 in [-2, 2] and
    a = lw - b + c (exact for the `probes` and `one_hot` rows: -1e4 +- k / 8 has 17 significant bits)."""
    rng = np.random.RandomState(seed)
    b = (rng.randint(-16, 17, size=lw.shape) / 8.0).astype(lw.dtype) if "+b" in which else None
    c = (rng.randint(-16, 17, size=lw.shape) / 8.0).astype(lw.dtype) if "-c" in which else None
    a = np.array(lw, copy=True)
    with np.errstate(all="ignore"):
        if c is not None:
            a = (a + c).astype(lw.dtype)
        if b is not None:
            a = (a - b).astype(lw.dtype)
    return a, b, c


# ---- profiles by case --------------------------------------------------------------------------------------------------
RANDOM_PROFILES = ("flat", "wide", "minus_inf_stretch", "dominant", "offset_up", "offset_down")
LONG_ROW_PROFILES = ("dominant", "probes", "probes_inf", "one_hot", "one_hot_inf")


def profile_names(K, ascending=False):
    names = (RANDOM_PROFILES + LONG_ROW_PROFILES[1:]) if K <= FLAT_MAX_PARTICLES else LONG_ROW_PROFILES
    return names + (("ascending", "descending") if ascending else ())


def one_hot_positions(B, K, L):
    """Row b's lone particle: the last of the first slice, then the first of the second, the last particle, ..."""
    spots = [min(K - 1, L - 1), min(K - 1, L), K - 1, 0, min(K - 1, 2 * L), 255 % K, 256 % K]
    return [spots[b % len(spots)] for b in range(B)]


def weights(name, B, K, dtype, seed, L=None, centre=False):
    """The profile `name` for a [B,K] row set; L the slice length (K7) that `probes` and `one_hot` aim at.  `centre` (K1's
    cases): the drawn profiles and the ascending ones are moved by an integer per row so that |lse| <= 1/2 — lse's metric
    divides by max(1, |lse|), and log K would otherwise hide a particle at K = 4100; the offset profiles keep theirs."""
    r = reductions
    if centre and not (name.startswith("offset") or name.startswith("probes") or name.startswith("one_hot")):
        return r.centred(weights(name, B, K, dtype, seed, L))
    if name == "probes":
        return r.probes(B, K, dtype, L=L)
    if name == "probes_inf":
        return r.probes(B, K, dtype, L=L, rest=-np.inf)
    if name == "one_hot":
        return r.one_hot(B, K, dtype, one_hot_positions(B, K, L or 64))
    if name == "one_hot_inf":
        return r.one_hot(B, K, dtype, one_hot_positions(B, K, L or 64), rest=-np.inf)
    return getattr(r, name)(B, K, dtype, seed)


def running_sum(name, lw, seed):
    """The `acc` operand of logweight_accumulate for a profile's rows: multiples of 1 / 8 in [-1/4, 1/4] (a flat row stays
    flat under them).  Under the offset profiles minus the offset and minus the integer nearest to the log-sum-exp of what
    is left, so that total = acc + lw is a centred flat row of order 1 in which a particle shows."""
    acc = np.random.RandomState(seed + 1).randint(-2, 3, size=lw.shape) / 8.0
    if name.startswith("offset"):
        back = (1 if name == "offset_up" else -1) * reductions.offset_shift(lw.dtype)
        acc = acc - back - np.rint(reductions.row_lse(lw.astype(np.float64) - back))[:, None]
    return acc.astype(lw.dtype)


def is_exact(name):
    return name.startswith("one_hot")


def case_seed(case, name, draw=0):
    return (case.B * 131 + case.K * 7 + sum(map(ord, name)) + 104729 * draw) % (2 ** 31 - 1)


# ---- the metric ----------------------------------------------------------------------------------------------------------
def _same_special(got, want):
    """Where `want` is not finite `got` has to be the same special value."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(want), np.isnan(got), got == want)


def error_floor_one(got, want):
    """lse, log_ess: max |got - want| / max(1, |want|); inf where a convention is missed."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    special = ~np.isfinite(want)
    with np.errstate(all="ignore"):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    err = np.where(special, np.where(_same_special(got, want), 0.0, np.inf), np.where(np.isfinite(got), err, np.inf))
    return float(err.max()) if err.size else 0.0


def error_relative(got, want, magnitude):
    """Mean, second moment, K1's gradient: max |got - want| / magnitude per element, no floor; where the magnitude is 0
    (or `want` is not finite) the output has to be exactly `want`: inf otherwise."""
    got, want, magnitude = [np.asarray(t, dtype=np.float64) for t in (got, want, magnitude)]
    exact = (magnitude == 0) | ~np.isfinite(want) | ~np.isfinite(magnitude)
    with np.errstate(all="ignore"):
        err = np.abs(got - want) / np.where(exact, 1.0, magnitude)
        same = np.where(np.isnan(want), np.isnan(got), got == want)
    err = np.where(exact, np.where(same, 0.0, np.inf), np.where(np.isfinite(got), err, np.inf))
    return float(err.max()) if err.size else 0.0
