"""tests/filter_model_expr.py, the model of the row filter's expression leaf, pinned on hand-written rows.  No GPU, no library."""
from decimal import Decimal

import pytest

import filter_model_expr as M
from orc_rust_amd.aggregate import col, lit

INT = {"a": "int", "b": "int", "c": "int"}
DEC = {"p": ("dec", 2), "q": ("dec", 7), "w": ("dec", 0), "z": ("dec", 20), "n": "int"}
FLT = {"x": "float", "y": "float"}
NAN, INF = float("nan"), float("inf")


def ev(lhs, op, rhs, row, schema):
    return M.evaluate(lhs, op, rhs, row, schema)


def test_classes_are_decided_over_both_sides():
    assert M.classify((col("a"), col("b") + 1), INT) == "int"
    assert M.classify((col("n"), col("p")), DEC) == "dec"
    assert M.classify((col("n"), lit(Decimal("1.5"))), DEC) == "dec"
    assert M.classify((col("x"), lit(1)), FLT) == "float"
    assert M.classify((lit(1), lit(2.0)), {}) == "float"
    with pytest.raises(ValueError):
        M.classify((col("x"), col("a")), dict(INT, **FLT))
    with pytest.raises(ValueError):
        M.classify((col("a"), lit(1.5)), INT)
    with pytest.raises(ValueError):
        M.classify((col("x"), lit(Decimal("1.5"))), FLT)


def test_int_rows_and_nulls():
    for row, want in [({"a": 1, "b": 2, "c": 3}, True), ({"a": 1, "b": 2, "c": 4}, False), ({"a": None, "b": 2, "c": 3}, None), ({"a": 1, "b": 2, "c": None}, None)]:
        assert ev(col("a") + col("b"), "=", col("c"), row, INT) == (want, False)
    row = {"a": -5, "b": 7, "c": 0}
    assert [ev(col("a"), op, col("b"), row, INT)[0] for op in ("=", "!=", "<", "<=", ">", ">=")] == [False, True, True, True, False, False]
    assert [ev(col("a"), op, col("a"), row, INT)[0] for op in ("=", "!=", "<", "<=", ">", ">=")] == [True, False, False, True, False, True]
    assert ev(col("b") - col("a"), ">", lit(11), row, INT) == (True, False) and ev(-col("b"), "<", col("a"), row, INT) == (True, False)
    # int64 columns cannot overflow 128 bits in one product; three of them can
    big = {"a": 2 ** 63 - 1, "b": 2 ** 63 - 1, "c": 2 ** 63 - 1}
    assert ev(col("a") * col("b"), ">", col("c"), big, INT) == (True, False)
    assert ev(col("a") * col("b") * col("c"), ">", col("c"), big, INT) == (None, True)
    assert ev(col("a") * col("b") * col("c"), ">", col("c"), dict(big, c=None), INT) == (None, False)  # the NULL comes first


def test_decimal_scales_and_the_final_rescale():
    # 1.50 against 1.5000000: equal whatever the scales
    row = {"p": 150, "q": 15000000, "w": 10 ** 37, "z": 5, "n": 2}
    assert ev(col("p"), "=", col("q"), row, DEC) == (True, False) and ev(col("p"), "<", col("q"), row, DEC) == (False, False)
    assert ev(col("p") * 2, "=", col("n") + 1, row, DEC) == (True, False)  # 3.00 = 3
    assert ev(col("p") * (1 - col("q")), "<", lit(0), row, DEC) == (True, False)  # 1.50 * (1 - 1.5) = -0.75
    # 10^37 at scale 0 against a scale-20 value: 10^57 leaves 128 bits, and the order is still exact
    assert ev(col("w"), ">", col("z"), row, DEC) == (True, False) and ev(col("z"), "<", col("w"), row, DEC) == (True, False)
    neg = dict(row, w=-(10 ** 37))
    assert ev(col("w"), "<", col("z"), neg, DEC) == (True, False) and ev(col("w"), "=", col("z"), neg, DEC) == (False, False)
    assert ev(col("w"), "!=", col("z"), neg, DEC) == (True, False) and ev(col("z"), "<=", col("w"), neg, DEC) == (False, False)
    # an operation INSIDE a side that leaves 128 bits: UNKNOWN, counted; under a NULL: UNKNOWN, not counted
    assert ev(col("w") * col("w"), ">", lit(0), row, DEC) == (None, True)
    assert ev(col("w") + col("z"), ">", lit(0), row, DEC) == (None, True)  # w is brought to scale 20 first: 10^57
    assert ev(col("w") * col("w"), ">", col("p"), dict(row, p=None), DEC) == (None, False)
    assert M.not3(None) is None and M.not3(True) is False
    with pytest.raises(ValueError):
        ev(col("z") * col("z"), ">", lit(0), row, DEC)  # scale 40


def test_float_rows():
    ops = ("=", "!=", "<", "<=", ">", ">=")
    assert [ev(col("x"), op, col("y"), {"x": NAN, "y": 1.0}, FLT)[0] for op in ops] == [False, True, False, False, False, False]
    assert [ev(col("x"), op, col("y"), {"x": 0.0, "y": -0.0}, FLT)[0] for op in ops] == [True, False, False, True, False, True]
    assert [ev(col("x"), op, col("y"), {"x": -INF, "y": INF}, FLT)[0] for op in ops] == [False, True, True, True, False, False]
    assert ev(col("x") * col("y"), ">", lit(1), {"x": 1e308, "y": 10.0}, FLT) == (True, False)  # inf, no overflow rule
    assert ev(col("x") - col("x"), "=", lit(0), {"x": INF, "y": 0.0}, FLT) == (False, False)  # inf - inf is NaN
    assert ev(col("x"), "<", col("y"), {"x": None, "y": 1.0}, FLT) == (None, False)
    assert ev(col("x") + 0.1, "=", lit(0.30000000000000004), {"x": 0.2, "y": 0.0}, FLT) == (True, False)


def test_kept_rows_and_the_overflow_count():
    rows = [{"w": 10 ** 37, "p": 1}, {"w": 3, "p": 100}, {"w": None, "p": 1}, {"w": -(10 ** 37), "p": 5}, {"w": 2, "p": None}]
    schema = {"w": ("dec", 0), "p": ("dec", 2)}
    assert M.kept(col("w") * col("w"), ">", col("p"), rows, schema) == ([1], 2)
    assert M.kept(col("w"), "<", col("p"), rows, schema) == ([3], 0)
