"""tests/div_model.py judged by what it does not use: `decimal` for the rounding of an exact quotient (exact halves of both signs
included), Python's own // and % for the floor rule, numpy's float64 division bit for bit; then the lowering of whole expressions
onto the existing models.  No GPU, no library."""
import decimal
import random
import struct

import numpy as np
import pytest

import agg_expr_model as AEM
import computed_model as CM
import div_model as M
from orc_rust_amd.aggregate import col, divide, lit, year

WIDE = decimal.Context(prec=120, rounding=decimal.ROUND_HALF_UP)  # (ROUND_HALF_UP: half away from zero, for both signs)
SCHEMA = {"a": "int", "b": "int", "d": "date", "p": ("dec", 2), "q": ("dec", 4), "x": "float", "y": "float"}
EDGES = [0, 1, -1, 2, -2, 3, 7, -7, 10, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, 2 ** 95, 2 ** 96 - 1, 2 ** 96,
         2 ** 96 + 1, 10 ** 38 - 1, 2 ** 127 - 1, -2 ** 127, -2 ** 127 + 1, -(10 ** 38 - 1), -2 ** 64, -2 ** 96]


def by_decimal(a, b, k):
    """round(a * 10^k / b) half away from zero through `decimal` alone"""
    q = WIDE.divide(WIDE.multiply(decimal.Decimal(a), decimal.Decimal(10) ** k), decimal.Decimal(b))
    return int(q.quantize(decimal.Decimal(1), context=WIDE))


def test_the_rounding_is_decimals_half_up():
    rnd = random.Random(7)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rnd.randint(-2 ** 100, 2 ** 100), rnd.randint(-2 ** 70, 2 ** 70)) for _ in range(500)]
    seen = 0
    for a, b in pairs:
        for k in (0, 1, 6, 19, 38):
            got = M.div_round(a, b, k)
            if b == 0 or not M.fits(a * 10 ** k):
                assert got is None
                continue
            want = by_decimal(a, b, k)
            assert got == (want if M.fits(want) else None), (a, b, k)
            seen += 1
    assert seen > 2000
    assert M.div_round(-2 ** 127, -1) is None and M.div_round(-2 ** 127, 1) == -2 ** 127 and M.div_round(2 ** 127 - 1, 1) == 2 ** 127 - 1


def test_exact_halves_of_both_signs_go_away_from_zero():
    for a, b, want in ((1, 2, 1), (-1, 2, -1), (1, -2, -1), (-1, -2, 1), (3, 2, 2), (-3, 2, -2), (5, 10, 1), (-5, 10, -1), (4, 10, 0), (-4, 10, 0), (6, -10, -1),
                       (2 ** 64 + 1, 2, 2 ** 63 + 1), (-(2 ** 64 + 1), 2, -(2 ** 63 + 1)), (2 ** 100 + 2 ** 64, 2 ** 65, 2 ** 35 + 1), (2 ** 126 + 2 ** 63, -2 ** 64, -(2 ** 62 + 1))):
        assert M.div_round(a, b) == want == by_decimal(a, b, 0), (a, b)
    assert M.div_round(125, 100, 1) == 13 and M.div_round(-125, 100, 1) == -13 and M.div_round(1, 3, 6) == 333333 and M.div_round(2, 3, 6) == 666667


def test_floor_division_and_modulo_are_pythons():
    rnd = random.Random(8)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rnd.randint(-2 ** 127, 2 ** 127 - 1), rnd.randint(-2 ** 90, 2 ** 90)) for _ in range(500)]
    for a, b in pairs:
        if b == 0:
            assert M.floor_div(a, b) is None and M.mod(a, b) is None
            continue
        q, r = M.floor_div(a, b), M.mod(a, b)
        assert r == a % b and (r == 0 or (r < 0) == (b < 0)) and abs(r) < abs(b)
        if (a, b) == (-2 ** 127, -1):
            assert q is None and r == 0
        else:
            assert q == a // b and a == q * b + r
    assert (M.floor_div(-7, 2), M.mod(-7, 2), M.floor_div(7, -2), M.mod(7, -2), M.floor_div(-7, -2), M.mod(-7, -2)) == (-4, 1, -4, -1, 3, -1)


def test_the_double_division_is_numpys_bit_for_bit():
    specials = [0.0, -0.0, 1.0, -1.0, 3.0, 0.1, 1e308, -1e308, 5e-324, 1e-308, float("inf"), float("-inf"), float("nan"), 2.0 ** 53 + 2, 1 / 3]
    rnd = random.Random(9)
    values = specials + [struct.unpack("<d", struct.pack("<Q", rnd.getrandbits(64)))[0] for _ in range(300)]
    a = np.array([x for x in values for _ in values], dtype=np.float64)
    b = np.array([y for _ in values for y in values], dtype=np.float64)
    with np.errstate(all="ignore"):
        want = a / b
    for x, y, w in zip(a.tolist(), b.tolist(), want.tolist()):
        assert CM.bits(M.float_div(x, y)) == CM.bits(w), (x, y)  # (a NaN's sign and payload too)


def test_the_scale_rule():
    assert [M.result_scale(s) for s in (0, 1, 2, 3, 30, 34, 35, 38)] == [6, 6, 6, 7, 34, 38, 38, 38]
    assert M.result_scale(5, 0) == 0 and M.power_of(2, 4) == 8 and M.power_of(0, 0) == 6 and M.power_of(4, 2, 2) == 0
    assert M.power_of(38, 38, 0) == 0 and M.power_of(0, 38, 0) == 38
    for sa, sb, s in ((4, 0, 3), (38, 0, 37), (0, 38, 1), (2, 37, None)):
        with pytest.raises(AEM.Refused) as e:
            M.power_of(sa, sb, s)
        assert e.value.status == "unsupported"


def test_whole_expressions_are_lowered_onto_the_existing_models():
    row = {"a": 7, "b": -2, "d": 9131, "p": 12345, "q": -50000, "x": 1.5, "y": 0.0}
    assert M.computed_type(col("a") / col("b"), SCHEMA) == (CM.DEC128, 6)  # int / int is a Decimal at scale 6
    assert M.computed_value(col("a") / col("b"), SCHEMA, row) == (-3500000, False)
    assert M.computed_type(col("p") / col("q"), SCHEMA) == (CM.DEC128, 6) and M.computed_value(col("p") / col("q"), SCHEMA, row) == (-24690000, False)
    assert M.computed_type(divide("p", "q", scale=1), SCHEMA) == (CM.DEC128, 1) and M.computed_value(divide("p", "q", scale=1), SCHEMA, row) == (-247, False)
    assert M.computed_type(col("a") // col("b") + col("a") % 4, SCHEMA) == (CM.INT64, 0)
    assert M.computed_value(col("a") // col("b") + col("a") % 4, SCHEMA, row) == (-4 + 3, False)
    assert M.computed_value(year("d") % 100 * col("p"), SCHEMA, row) == (95 * 12345, False)
    assert M.computed_value(col("a") / (col("b") + 2), SCHEMA, row) == (None, True)           # a zero divisor overflows
    assert M.computed_value(col("a") % (col("b") + 2), SCHEMA, row) == (None, True)
    assert M.computed_value(col("a") / col("b"), SCHEMA, dict(row, b=None)) == (None, False)  # NULL comes first
    assert M.computed_value(0 * (col("a") / (col("b") + 2)), SCHEMA, row) == (None, True)     # never a silent value
    assert M.computed_type(col("x") / col("y"), SCHEMA) == (CM.FLOAT64, 0) and M.computed_value(col("x") / col("y"), SCHEMA, row) == (float("inf"), False)
    assert M.agg_row(col("p") / 3 + col("q"), SCHEMA, row) == 41150000 - 5000000 and M.agg_scale(col("p") / 3 + col("q"), SCHEMA) == 6
    assert M.filter_leaf(col("a") / col("b"), "<", lit(decimal.Decimal("-3.4")), row, SCHEMA) == (True, False)
    assert M.filter_leaf(col("a") % 2, "=", 1, row, SCHEMA) == (True, False) and M.filter_leaf(col("a") // 0, "=", 1, row, SCHEMA) == (None, True)
    for bad, status in ((col("p") // 2, "mismatched"), (col("a") % col("q"), "mismatched"), (col("x") // 2.0, "mismatched"), (divide("q", "a", scale=3), "unsupported")):
        with pytest.raises(AEM.Refused) as e:
            M.computed_value(bad, SCHEMA, row)
        assert e.value.status == status, bad
