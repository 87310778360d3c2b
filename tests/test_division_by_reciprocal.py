"""The item form of the fused propagation launch divides a particle's three sums of squares by 2 s^2 through
reciprocals formed once per workgroup (aesmc_amd/csrc/linear_gaussian_item.hip: `item_quotient`): with r = RN(1 / d),

    q0 = n r,    e = fma(-d, q0, n),    q = fma(e, r, q0)

must be the correctly rounded quotient n / d — the bits of the IEEE division the other path keeps — for every numerator
and divisor the kernel's guard lets through, and the guard must turn away what the form does not cover (subnormal
numerators, zeros whose sign the form loses, infinities, NaNs).  The log-weight these quotients go into is the
reference's Normal log-density (aesmc/state.py:98 through torch.distributions): -(x - mu)^2 / (2 s^2) summed.

numpy has no fused multiply-add: float32 `fma` is restated exactly (the product of two float32 values is exact in
float64; the sum is rounded to odd there before the one rounding to float32) and that restatement is itself held to
rational arithmetic on a sample; the correctly rounded quotient is settled in integers.
"""
from fractions import Fraction

import numpy as np

# the kernel's guard (linear_gaussian_item.hip: kRecipNumLo .. kRecipDivHi), as bit patterns of float32
NUM_LO, NUM_HI = 0x21800000, 0x5d800000      # 2^-60, 2^60
DIV_LO, DIV_HI = 0x36000000, 0x49000000      # 2^-19, 2^19
SCALES = [0.05, 0.1, 0.3, 0.45, 0.5, 0.7, 0.9, 1.0, 1.3, 2.0]


def bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def numerator_guard(q):
    """What the kernel asks of a sum of squares q (the numerator is -q): one unsigned comparison pair on the bit pattern —
    a NaN, an infinity, a zero, a subnormal and anything with the sign bit set lie outside."""
    u = bits(q).astype(np.int64)
    return (u >= NUM_LO) & (u <= NUM_HI)


def divisor_guard(d):
    u = bits(d).astype(np.int64)
    return (u - DIV_LO) % (1 << 32) <= DIV_HI - DIV_LO      # the kernel's single unsigned comparison


def fma32(a, b, c):
    """RN_float32(a b + c) with one rounding."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                                    # exact: 24 + 24 significant bits
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                # TwoSum: p + c == s + err exactly
    raw = np.asarray(s).view(np.int64)
    nudge = (err != 0) & ((raw & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)                  # towards the larger magnitude: the bit pattern grows
    raw = raw + np.where(nudge & away, 1, 0) - np.where(nudge & ~away, 1, 0)
    return raw.view(np.float64).astype(np.float32)      # (53 >= 24 + 2 bits rounded to odd: the second rounding is the only one)


def quotient_by_reciprocal(n, d):
    n, d = np.asarray(n, dtype=np.float32), np.asarray(d, dtype=np.float32)
    r = np.float32(1.0) / d                      # one IEEE division per divisor
    q0 = n * r
    e = fma32(-d, q0, n)
    return fma32(e, r, q0)


def split(v):
    """v = m 2^e with |m| an integer of exactly 24 bits (normal float32 values)."""
    m, e = np.frexp(np.asarray(v, dtype=np.float32).astype(np.float64))
    return np.round(m * (1 << 24)).astype(np.int64), e.astype(np.int64) - 24


def is_correctly_rounded(q, n, d):
    """q == RN(n / d), settled in integers: with 24-bit integers m, n - q d = (m_n 2^s - m_q m_d) 2^E and half a unit in the
    last place of q times d is m_d 2^E / 2 — below a power of two the spacing halves."""
    mn, en = split(n)
    md, ed = split(d)
    mq, eq = split(q)
    sign = np.sign(mn) * np.sign(md)
    mn, md, mq_abs = np.abs(mn), np.abs(md), np.abs(mq)
    ok = np.sign(mq) == sign
    shift = en - (eq + ed)                       # 22 .. 25 when q is anywhere near n / d
    ok &= (shift >= 0) & (shift <= 26)
    resid = (mn << np.clip(shift, 0, 26)) - mq_abs * md      # < 2^51: exact in int64
    below = resid < 0                            # the quotient lies below |q|
    half = np.where(below & (mq_abs == 1 << 23), 4, 2)
    ok &= half * np.abs(resid) <= md
    assert not np.any(ok & (half * np.abs(resid) == md) & (resid != 0)), "a tie: cannot happen in a division"
    return ok


def samples():
    rng = np.random.RandomState(20240)
    divisors = [np.float32(2.0) * (np.float32(s) * np.float32(s)) for s in SCALES]      # the kernel's own expression
    divisors += list(np.exp2(rng.uniform(-19, 19, 54)).astype(np.float32))
    divisors += [np.float32(2.0 ** -19), np.float32(2.0 ** 19)]
    divisors = np.array(divisors, dtype=np.float32)
    assert divisor_guard(divisors).all()
    exponents = np.arange(-60, 60)
    edge = np.concatenate([np.exp2(exponents.astype(np.float64)),                              # all-zero mantissas
                           np.exp2(exponents.astype(np.float64)) * (2.0 - 2.0 ** -23),         # all-one mantissas
                           [2.0 ** 60]]).astype(np.float32)
    per_exponent = 12
    mant = 1.0 + rng.randint(0, 1 << 23, size=(len(exponents), per_exponent)) / float(1 << 23)
    rand = (np.exp2(exponents.astype(np.float64))[:, None] * mant).astype(np.float32).ravel()
    nums = np.concatenate([edge, rand])
    assert numerator_guard(nums).all()
    n, d = np.meshgrid(nums, divisors, indexing="ij")
    return -n.ravel(), d.ravel()                 # the kernel's numerators are -q


def test_fma_restatement_is_the_fused_multiply_add():
    rng = np.random.RandomState(3)
    a = (rng.randn(3000) * np.exp2(rng.randint(-30, 30, 3000))).astype(np.float32)
    b = (rng.randn(3000) * np.exp2(rng.randint(-30, 30, 3000))).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.randn(3000) * np.exp2(rng.randint(-30, 2, 3000)))).astype(np.float32)
    got = fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(exact - Fraction(float(g))) <= abs(exact - Fraction(float(lo))), (x, y, z, g)
        assert abs(exact - Fraction(float(g))) <= abs(exact - Fraction(float(hi))), (x, y, z, g)


def test_two_fused_corrections_give_the_division_bits_inside_the_guard():
    n, d = samples()
    assert n.size >= 100000
    q = quotient_by_reciprocal(n, d)
    good = is_correctly_rounded(q, n, d)
    assert good.all(), "{} of {} quotients are not correctly rounded, first (n, d, q): {}".format(
        int((~good).sum()), n.size, (n[~good][:3], d[~good][:3], q[~good][:3]))
    # and the plain float32 division of the other path agrees bit for bit (numpy's is IEEE)
    assert (n / d).view(np.uint32).tolist() == q.view(np.uint32).tolist()


def test_the_guard_turns_away_what_the_form_does_not_cover():
    """Subnormal, zero, infinite and NaN sums of squares: the guard rejects each, so the kernel divides them — that
    rejection, not luck, keeps them exact (the form itself loses the sign of a zero quotient and breaks on the rest)."""
    planted = np.array([1e-45, 1e-39, 0.0, -0.0, np.inf, np.nan, -np.nan, 2.0 ** -61, np.nextafter(np.float32(2.0 ** 60), np.float32(np.inf)),
                        3e38], dtype=np.float32)
    assert not numerator_guard(planted).any()
    assert numerator_guard(np.array([2.0 ** -60, 1.0, 2.0 ** 60], dtype=np.float32)).all()
    outside = np.array([0.0, -1.0, np.inf, np.nan, 2.0 ** -20, np.nextafter(np.float32(2.0 ** 19), np.float32(np.inf)), 1e-40],
                       dtype=np.float32)
    assert not divisor_guard(outside).any()
    # what the rejection protects against: a zero sum of squares gives -0 / d = -0, the form gives +0 ...
    d = np.float32(0.5)
    assert np.signbit(np.float32(-0.0) / d) and not np.signbit(quotient_by_reciprocal(np.float32(-0.0), d))
    # ... and an infinite one gives -inf, the form NaN (inf - inf in the residual)
    with np.errstate(invalid="ignore"):
        assert np.isnan(quotient_by_reciprocal(np.float32(-np.inf), d)) and np.float32(-np.inf) / d == -np.inf
