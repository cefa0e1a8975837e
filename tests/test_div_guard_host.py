"""The guards of STRICT's divisions by a known divisor, proven on the CPU with the exact model of tests/div_model.py.

Wherever a guard of ns3d_kernels.hip says "fast path", the reciprocal sequence must equal the correctly rounded quotient —
RN(x/d), or RN(RN(x/d)/d) for the two-division forms — bit for bit, for EVERY divisor the host admission recip_ok
(ns3d_api.cpp) lets through.  The constants of both are read from the sources, so the test follows them.

Divisors per element type: the reference's spacings, 3 (DIV_3), the admitted divisors nearest each end of recip_ok's range
(a plain one and one whose significand is all ones but the last bit) and a seeded log-uniform sample of the admitted range.
Dividends per divisor: quotients within four binades of each guard bound, on both sides; half random, half planted next to
representable numbers and rounding midpoints (x = RN(q_c·d) moved by −3…+3 steps, the device self-test's planting).
"""
import math
import random

import numpy as np
import pytest

import div_model as M
from div_model import F32, F64

FMTS = [F32, F64]
NP = {"f32": np.float32, "f64": np.float64}
REFERENCE_SPACINGS = [1.0 / 63, 0.6 / 38, 1.0 / 255, 0.6 / 153, 1.0 / 512, 0.7 / 5]
SMALL = 1.3 * 2.0 ** -19          # the divisor of the recorded counter-example


def _divisors(fmt):
    """[(bits of (T)d, weight)]: weight scales the number of dividends (the ends of the admitted range get the most)."""
    rng = random.Random(20240917)
    lo = max(M.CONST["recip_f64"][0], M.CONST["recip_f32"][0])
    hi = min(M.CONST["recip_f64"][1], M.CONST["recip_f32"][1])
    ds = [(d, 1) for d in REFERENCE_SPACINGS[:5]] + [(3.0, 1), (SMALL, 6)] + [(d, 6) for d in M.admitted_extremes(fmt)]
    while len(ds) < 27:
        d = math.exp(rng.uniform(math.log(lo), math.log(hi)))
        d = M.from_bits(fmt, M.to_bits(fmt, d))             # a sample of the TYPE's divisors
        if M.recip_ok(d):
            ds.append((d, 1))
    for d, _ in ds:
        assert M.recip_ok(d), d
    return [(M.divisor_of(fmt, d), w) for d, w in ds]


def _fmt_x(fmt, b):
    return "%r (bits %#x)" % (M.from_bits(fmt, b), b)


def test_constants_come_from_the_sources():
    """One source of truth: the model holds what the two files say, and text that is not found raises."""
    for name in ("DivLim", "Div2Lim", "ValLim"):
        for fmt in FMTS:
            lo, hi = M.CONST[name][fmt.name]
            assert 0 < lo < hi < fmt.inf
    assert M.CONST["recip_f64"][0] < M.CONST["recip_f64"][1] and M.CONST["recip_f32"][0] < M.CONST["recip_f32"][1]
    with pytest.raises(RuntimeError, match="not found"):
        M._find("static constexpr double low = 1;", r"lo\s*=\s*0x1p", "DivLim<double>", "nowhere")


@pytest.mark.parametrize("fmt", FMTS, ids=repr)
def test_model_arithmetic_equals_the_hardware(fmt):
    """The model's RN against this machine's IEEE arithmetic (NumPy, in the element type): products, differences and quotients over
    the whole exponent range, subnormal and overflowing results included, signed zeros and specials."""
    rng = random.Random(7)
    T = NP[fmt.name]
    special = [0, fmt.sign_bit, 1, fmt.sign_bit | 1, fmt.hidden - 1, fmt.hidden, fmt.inf - 1, fmt.inf, fmt.inf | fmt.sign_bit, fmt.nan]
    pool = special + [M._rand_in_binade(fmt, rng, rng.randrange(fmt.qmin, fmt.bias + 1)) for _ in range(300)]
    pool += [rng.getrandbits(fmt.p - 1) | (rng.getrandbits(1) * fmt.sign_bit) for _ in range(40)]     # subnormals
    arr = lambda b: np.array([M.from_bits(fmt, b)], dtype=T)

    def same(got, want):
        want = M.to_bits(fmt, want[0]) if not np.isnan(want[0]) else fmt.nan
        return (M.is_nan(fmt, got) and want == fmt.nan) or got == want

    with np.errstate(all="ignore"):
        for _ in range(6000):
            a, b = rng.choice(pool), rng.choice(pool)
            if rng.random() < 0.5:                               # operands of nearby magnitude: cancellation, quotients near 1
                b = M._rand_in_binade(fmt, rng, M._exponent(fmt, a) + rng.randrange(-2, 3)) if M.is_finite(fmt, a) and not M.is_zero(fmt, a) else b
            assert same(M.mul(fmt, a, b), arr(a) * arr(b)), ("mul", a, b)
            assert same(M.div(fmt, a, b), arr(a) / arr(b)), ("div", a, b)
            if M.is_finite(fmt, a) and M.is_finite(fmt, b):
                assert same(M.sub(fmt, a, b), arr(a) - arr(b)), ("sub", a, b)
                # fma(a, 1, −b) must be the same single rounding
                assert M.fma(fmt, a, M.to_bits(fmt, 1.0), M.neg(fmt, b)) == M.sub(fmt, a, b)


def test_fma_is_one_rounding():
    """fma against exact rational arithmetic on cases where two roundings differ from one."""
    from fractions import Fraction
    rng = random.Random(11)
    for fmt in FMTS:
        for _ in range(2000):
            a, b = (M._rand_in_binade(fmt, rng, rng.randrange(-30, 30)) for _ in range(2))
            c = M.neg(fmt, M.mul(fmt, a, b))                     # a·b + c = the rounding error of the product: exact, tiny
            got = M.fma(fmt, a, b, c)
            exact = Fraction(M.from_bits(fmt, a)) * Fraction(M.from_bits(fmt, b)) + Fraction(M.from_bits(fmt, c))
            assert Fraction(M.from_bits(fmt, got)) == exact


def test_recip_ok_admits_the_reference_spacings_and_nothing_degenerate():
    for d in REFERENCE_SPACINGS + [3.0, SMALL]:
        assert M.recip_ok(d), d
    for d in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -101, 2.0 ** 101, 2.0 ** -20, 2.0 ** 20, float(np.nextafter(2.0, 0.0)),
              float(np.nextafter(np.float32(2.0), np.float32(0.0)))):
        assert not M.recip_ok(d), d
    for fmt in FMTS:
        for d in M.admitted_extremes(fmt):
            assert M.recip_ok(d) and M.from_bits(fmt, M.to_bits(fmt, d)) == d


def test_recorded_counter_example_f32():
    """d = float32(1.3·2⁻¹⁹) is admitted; x = 7.336370446077286e-36 has the quotient 2.9587e-30 ≈ 2⁻⁹⁸·⁰⁵.  With the guard
    |q| > 2⁻¹⁰⁰ the sequence ran there and returned 2.958746928646829e-30, one step below RN(x/d) = 2.958747116725925e-30:
    q·d is a multiple of ulp(q)·ulp(d) = 2⁻¹²¹·2⁻⁴² < 2⁻¹⁴⁹, so the residual e was rounded.  The guard must either refuse
    this dividend or the sequence must be exact."""
    fmt = F32
    assert M.recip_ok(SMALL)
    d = M.divisor_of(fmt, SMALL)
    x = M.to_bits(fmt, 7.336370446077286e-36)
    r = M.recip(fmt, d)
    want = M.div(fmt, x, d)
    assert M.from_bits(fmt, want) == float(np.float32(7.336370446077286e-36) / np.float32(SMALL)) == 2.958747116725925e-30
    assert M.from_bits(fmt, M.seq_div(fmt, x, d, r)) == 2.958746928646829e-30          # the sequence itself IS wrong here
    fast, got = M.div_by_known(fmt, x, d, r)
    assert not fast or got == want, \
        "div_by_known(float) takes the fast path for x = 7.336370446077286e-36, d = float32(1.3*2^-19) and returns %r, RN(x/d) = %r" % (
            M.from_bits(fmt, got), M.from_bits(fmt, want))
    for xs in (x, M.neg(fmt, x)):                                                         # and every value is the quotient's
        assert M.div_by_known(fmt, xs, d, r)[1] == M.div(fmt, xs, d)


@pytest.mark.parametrize("fmt", FMTS, ids=repr)
def test_single_division_guard_is_exact_over_the_admitted_range(fmt):
    """div_by_known: fast path ⇒ RN(x/d); both paths ⇒ the plain quotient's bits (±0/d = ±0 through `q1 = x`)."""
    rng = random.Random(101)
    lim = M.CONST["DivLim"][fmt.name]
    fast_n = slow_n = 0
    for d, weight in _divisors(fmt):
        r = M.recip(fmt, d)
        for bound in lim:
            for x in M.dividends_for_quotient_bound(fmt, rng, d, bound, 700 * weight):
                fast, got = M.div_by_known(fmt, x, d, r)
                want = M.div(fmt, x, d)
                assert got == want, "%s: d = %s, x = %s: %s path gives %s, RN(x/d) = %s" % (
                    fmt, _fmt_x(fmt, d), _fmt_x(fmt, x), "fast" if fast else "plain", _fmt_x(fmt, got), _fmt_x(fmt, want))
                fast_n += fast; slow_n += not fast
        for x in (0, fmt.sign_bit):
            assert M.div_by_known(fmt, x, d, r) == (False, x)
    assert fast_n > 20000 and slow_n > 20000                     # both sides of the bounds were really sampled


@pytest.mark.parametrize("fmt", FMTS, ids=repr)
def test_two_division_guards_are_exact_over_the_admitted_range(fmt):
    """div2_known where its `ok` holds, and div2_known_nochk on the same dividends (what val_ok promises it): RN(RN(x/d)/d)."""
    rng = random.Random(202)
    lim = M.CONST["Div2Lim"][fmt.name]
    ok_n = no_n = 0
    for d, weight in _divisors(fmt):
        r = M.recip(fmt, d)
        for bound in lim:
            for x in M.dividends_for_dividend_bound(fmt, rng, d, bound, 240 * weight):
                ok, got = M.div2_known(fmt, x, d, r)
                ok_n += ok; no_n += not ok
                if not ok:
                    continue
                want = M.div2_exact(fmt, x, d)
                assert got == want, "%s div2_known: d = %s, x = %s: %s, RN(RN(x/d)/d) = %s" % (
                    fmt, _fmt_x(fmt, d), _fmt_x(fmt, x), _fmt_x(fmt, got), _fmt_x(fmt, want))
                assert M.div2_known_nochk(fmt, x, d, r) == want, "%s div2_known_nochk: d = %s, x = %s" % (fmt, _fmt_x(fmt, d), _fmt_x(fmt, x))
        for x in (0, fmt.sign_bit):                              # ±0: z ? x, and the copysign
            assert M.div2_known(fmt, x, d, r) == (True, x) and M.div2_known_nochk(fmt, x, d, r) == x == M.div2_exact(fmt, x, d)
    assert ok_n > 5000 and no_n > 5000


@pytest.mark.parametrize("fmt", FMTS, ids=repr)
def test_val_ok_values_keep_second_differences_inside_div2lim(fmt):
    """The per-value guard: for any three values that pass val_ok, (e − c) − (c − w) is zero or inside Div2Lim — so
    div2_known_nochk may run unguarded on it — with values at and around both ends of ValLim, equal and opposite neighbours,
    values one step apart, and zeros of both signs."""
    rng = random.Random(303)
    lo, hi = M.CONST["ValLim"][fmt.name]
    d2 = M.CONST["Div2Lim"][fmt.name]
    assert not M.val_ok(fmt, lo) and not M.val_ok(fmt, hi) and M.val_ok(fmt, lo + 1) and M.val_ok(fmt, hi - 1)
    for bad in (fmt.inf, fmt.nan, 1, lo - 1, hi + 1):
        assert not M.val_ok(fmt, bad)
    edge = [0, lo + 1, lo + 2, lo + 3, hi - 1, hi - 2, hi - 3, M.to_bits(fmt, 1.0), M.to_bits(fmt, 1.0) + 1]
    edge += [M._rand_in_binade(fmt, rng, M._exponent(fmt, lo) + rng.randrange(0, 4), 0) for _ in range(6)]
    edge += [M._rand_in_binade(fmt, rng, M._exponent(fmt, hi) - 1 - rng.randrange(0, 4), 0) for _ in range(6)]
    edge = [v for v in edge if M.val_ok(fmt, v)]
    pool = edge + [v | fmt.sign_bit for v in edge]
    triples = [(w, c, e) for w in pool for c in pool for e in pool]
    rng.shuffle(triples)
    divisors = [d for d, _ in _divisors(fmt)]
    nonzero = 0
    for k, (w, c, e) in enumerate(triples[:40000]):
        x = M.second_difference(fmt, w, c, e)
        assert M.is_zero(fmt, x) or M._between(fmt, M.fabs(fmt, x), d2), \
            "%s: (e−c)−(c−w) = %s for w, c, e = %s, %s, %s leaves Div2Lim" % (fmt, _fmt_x(fmt, x), _fmt_x(fmt, w), _fmt_x(fmt, c), _fmt_x(fmt, e))
        nonzero += not M.is_zero(fmt, x)
        if k % 8 == 0:                                           # and the unguarded form is then exact, signed zeros included
            d = divisors[(k // 8) % len(divisors)]
            assert M.div2_known_nochk(fmt, x, d, M.recip(fmt, d)) == M.div2_exact(fmt, x, d), (fmt, _fmt_x(fmt, d), _fmt_x(fmt, x))
    assert nonzero > 20000
