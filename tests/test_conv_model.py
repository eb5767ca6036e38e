"""tests/conv_model.py, the model of the conversions (include/orcgpu.h: CONVERSIONS), judged by independent references:
float(fractions.Fraction(u, 10**s)) for to-double; decimal.Decimal(x) -- exact from a float -- quantized under a context of 80 digits
with ROUND_HALF_UP (half away from zero), ROUND_FLOOR, ROUND_CEILING and ROUND_DOWN for the others; math.floor / ceil / trunc for
doubles.  No GPU."""
import decimal
import math
import struct
from fractions import Fraction

import pytest

import conv_model as M
from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import cast, ceil, col, decimal_, floor, lit, round_, trunc, when, year

CTX = decimal.Context(prec=80)
MODES = {M.HALF_AWAY: decimal.ROUND_HALF_UP, M.FLOOR: decimal.ROUND_FLOOR, M.CEIL: decimal.ROUND_CEILING, M.TRUNC: decimal.ROUND_DOWN}
NAN, INF = float("nan"), float("inf")
# |unscaled| around the bounds of the fast path (2^53), of one word (2^64) and of a Decimal128 (10^38 - 1), ties at .5 of both signs
UNSCALED = sorted({s * (b + d) for s in (1, -1) for b in (2 ** 53, 2 ** 64, 10 ** 38 - 1) for d in (-2, -1, 0, 1, 2) if abs(b + d) < 10 ** 38} |
                  {0, 1, -1, 5, -5, 15, -15, 25, -25, 50, -50, 149, 150, 151, -149, -150, -151, 250, -250, 2 ** 63 - 1, -2 ** 63, 2 ** 127 - 1, -2 ** 127,
                   12345678901234567890123456789012345678, 5 * 10 ** 37, -5 * 10 ** 37, 10 ** 22, 10 ** 23, 3 * 10 ** 22 + 1})
SCALES = (0, 1, 2, 22, 23, 38)
DOUBLES = [0.1, 0.5, 2.5, -2.5, 1.5, -1.5, 0.49999999999999994, 1e22, 1e23, 5e-324, -5e-324, 2.0 ** 63, -2.0 ** 63, 2.0 ** 63 - 1024, -2.0 ** 63 - 2048, 9.999e37, 1e38,
           -1e38, NAN, INF, -INF, -0.0, 0.0, 0.005, 1.005, -0.125, 123456.789, 2.0 ** 52 + 0.5, 2.0 ** 53, 1e-40, 4.35, -4.35]
TARGETS = (0, 2, 22, 23, 38)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.mark.parametrize("s", SCALES)
def test_to_double_is_the_nearest_double_of_the_exact_rational(s):
    for u in UNSCALED:
        want = float(Fraction(u, 10 ** s))
        assert bits(M.to_f64(u, s)) == bits(want), (u, s)
        # ... and the reference itself is what decimal says: no double lies nearer
        exact = CTX.divide(decimal.Decimal(u), decimal.Decimal(10) ** s)
        for other in (math.nextafter(want, INF), math.nextafter(want, -INF)):
            assert abs(CTX.subtract(decimal.Decimal(want), exact)) <= abs(CTX.subtract(decimal.Decimal(other), exact)), (u, s)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_rescale_rounds_as_decimal_quantize(mode):
    for u in UNSCALED:
        for k in (1, 2, 10, 22, 23, 38):
            want = int(CTX.scaleb(decimal.Decimal(u), -k).quantize(decimal.Decimal(1), rounding=MODES[mode], context=CTX))
            assert M.rescale(u, k, mode) == want, (u, k, mode)


@pytest.mark.parametrize("t", TARGETS)
def test_double_to_decimal_is_the_exact_value_rounded_half_away(t):
    for x in DOUBLES:
        got = M.f64_to_dec(x, t)
        if math.isnan(x) or math.isinf(x):
            assert got is M.OVER, x
            continue
        want = int(CTX.scaleb(decimal.Decimal(x), t).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP, context=CTX))
        assert (got is M.OVER) == (abs(want) >= 10 ** 38), (x, t)
        if got is not M.OVER:
            assert got == want, (x, t)
    assert M.f64_to_dec(-0.0, t) == 0 and M.f64_to_dec(2.5, 0) == 3 and M.f64_to_dec(-2.5, 0) == -3


def test_double_to_int64_truncates_and_overflows_outside_int64():
    for x in DOUBLES:
        got = M.f64_to_i64(x)
        if math.isnan(x) or math.isinf(x):
            assert got is M.OVER
            continue
        want = int(decimal.Decimal(x).to_integral_value(rounding=decimal.ROUND_DOWN))
        assert (got is M.OVER) == (not -2 ** 63 <= want < 2 ** 63), x
        if got is not M.OVER:
            assert got == want == math.trunc(x)
    assert M.f64_to_i64(2.0 ** 63) is M.OVER and M.f64_to_i64(-2.0 ** 63) == -2 ** 63 and M.f64_to_i64(2.0 ** 63 - 1024) == 2 ** 63 - 1024


def test_double_roundings_are_c_round_floor_ceil_trunc():
    for x in DOUBLES:
        for mode, ref in ((M.FLOOR, math.floor), (M.CEIL, math.ceil), (M.TRUNC, math.trunc)):
            got = M.f64_round(x, mode)
            if math.isnan(x) or math.isinf(x):
                assert bits(got) == bits(x)
            else:
                assert got == float(ref(x)), (x, mode)
        got = M.f64_round(x, M.HALF_AWAY)
        if math.isnan(x) or math.isinf(x):
            assert bits(got) == bits(x)
        else:
            want = int(decimal.Decimal(x).to_integral_value(rounding=decimal.ROUND_HALF_UP))
            assert got == float(want) and math.copysign(1, got) == math.copysign(1, x), x
    assert M.f64_round(0.49999999999999994, M.HALF_AWAY) == 0.0 and M.f64_round(2.5, M.HALF_AWAY) == 3.0 and M.f64_round(-2.5, M.HALF_AWAY) == -3.0
    assert bits(M.f64_round(-0.5, M.CEIL)) == bits(-0.0)


SCHEMA = {"l": "int", "p": ("dec", 2), "w": ("dec", 10), "x": "float", "d": "int"}


def test_types_are_decided_per_node():
    T = lambda e: M.type_of(e, SCHEMA)
    assert T(cast("p", "float64") * col("x")) == ("float", 0)
    assert T(cast(col("x") * 100, decimal_(2)) + col("p")) == ("dec", 2)
    assert T(floor("p")) == ("dec", 0) and T(round_("w", 4)) == ("dec", 4) and T(round_("p", 4)) == ("dec", 2) and T(round_("l", 3)) == ("int", 0)
    assert T(cast(floor(col("p") / 1000), "int64")) == ("int", 0)
    assert T(year(cast("x", "int64"))) == ("int", 0) and T(year(floor("p"))) == ("int", 0)
    assert T(when(col("x") > 0, cast("x", "int64"), floor("p"))) == ("dec", 0)
    assert T(cast("l", "float64") / 3) == ("float", 0) and T(col("l") / 3) == ("dec", 6)
    assert T(cast("l", "int64") % 7) == ("int", 0)
    for bad, status in ((cast("p", "float64") + col("p"), "mismatched"), (round_("x", 2), "unsupported"), (year(floor("x")), "mismatched"),
                        (floor("x") % 2, "mismatched"), (year(round_("p", 1)), "mismatched")):
        with pytest.raises(M.AEM.Refused) as r:
            T(bad)
        assert r.value.status == status, bad


def test_rows_null_overflow_and_the_untaken_branch():
    row = {"l": 7, "p": -12345, "w": 15 * 10 ** 9, "x": float("nan"), "d": 0}
    V = lambda e, r=row: M.computed_value(e, SCHEMA, r)
    assert V(cast("p", "int64")) == (-123, False) and V(floor("p")) == (-124, False) and V(ceil("p")) == (-123, False) and V(trunc("p")) == (-123, False)
    assert V(round_("p", 1)) == (-1235, False) and V(round_("w", 0)) == (2, False)
    assert V(cast("x", "int64")) == (None, True) and V(cast("x", decimal_(2))) == (None, True)
    assert V(when(col("x") > 0, cast("x", "int64"), floor("p"))) == (-124, False)  # NaN > 0 is FALSE: the cast that overflows is not taken
    assert V(cast("l", "float64") / 3) == (7.0 / 3.0, False)
    assert V(cast("p", "float64")) == (-123.45, False)
    assert V(cast("l", decimal_(38))) == (None, True)  # 7 * 10^38 leaves the type
    assert V(cast("p", "float64"), dict(row, p=None)) == (None, False)
    assert V(cast(lit(2 ** 62) * 4, "int64")) == (None, True)
