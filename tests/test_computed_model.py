"""tests/computed_model.py against hand cases: the output type and scale, the NULL rule, the three overflow cases and the count,
the doubles bit for bit.  No GPU, no library."""
import math

import pytest

import agg_expr_model as AEM
import computed_model as M
from orc_rust_amd.aggregate import col, lit

SCHEMA = {"a": "int", "b": "int", "d": "date", "p": ("dec", 2), "q": ("dec", 2), "w": ("dec", 0), "x": "float", "y": "float", "s": "string", "t": "bool"}


def test_output_types_and_scales():
    assert M.output_type(col("a") + col("b"), SCHEMA) == (M.INT64, 0)
    assert M.output_type(col("d") - col("a"), SCHEMA) == (M.INT64, 0)  # a Date is int64 days
    assert M.output_type(col("p") * col("q"), SCHEMA) == (M.DEC128, 4)  # 2 x 2 gives 4
    assert M.output_type(col("p") + col("w"), SCHEMA) == (M.DEC128, 2)
    assert M.output_type(col("p") * (1 - col("q")), SCHEMA) == (M.DEC128, 4)
    assert M.output_type(col("a") * col("p"), SCHEMA) == (M.DEC128, 2)
    assert M.output_type(col("x") * col("y") + 1.5, SCHEMA) == (M.FLOAT64, 0)
    for e in (col("s") + 1, col("t") + 1, col("x") + col("a"), lit(1) + lit(2)):
        with pytest.raises(AEM.Refused):
            M.output_type(e, SCHEMA)


def test_int64_edges():
    e = col("a") + col("b")
    assert M.eval_value(e, SCHEMA, {"a": 2 ** 63 - 1, "b": 1}) == (None, True)  # NULL and counted
    assert M.eval_value(e, SCHEMA, {"a": 2 ** 63 - 1, "b": 0}) == (2 ** 63 - 1, False)
    assert M.eval_value(col("a") - col("b"), SCHEMA, {"a": -2 ** 63, "b": 0}) == (-2 ** 63, False)  # fits
    assert M.eval_value(col("a") - col("b"), SCHEMA, {"a": -2 ** 63, "b": 1}) == (None, True)
    assert M.eval_value(-col("a"), SCHEMA, {"a": -2 ** 63}) == (None, True)
    assert M.eval_value(e, SCHEMA, {"a": None, "b": 1}) == (None, False)  # NULL, not counted
    # an intermediate past int64 that comes back fits: only the result is checked against int64
    assert M.eval_value(col("a") * col("b") - col("a") * col("b") + 7, SCHEMA, {"a": 2 ** 62, "b": 4}) == (7, False)


def test_decimal_edges():
    e = col("w") * col("a")
    assert M.eval_value(e, SCHEMA, {"w": 10 ** 19 - 1, "a": 10 ** 19 + 1}) == (10 ** 38 - 1, False)  # exactly 10^38 - 1
    assert M.eval_value(e, SCHEMA, {"w": 10 ** 19, "a": 10 ** 19}) == (None, True)  # exactly 10^38
    assert M.eval_value(e, SCHEMA, {"w": -(10 ** 19), "a": 10 ** 19}) == (None, True)
    assert M.eval_value(col("p") * col("q"), SCHEMA, {"p": 150, "q": 250}) == (37500, False)  # 1.50 * 2.50 = 3.7500
    # -(-2^127): the operation leaves 128 bits
    assert M.eval_value(-(col("w") * col("a")), SCHEMA, {"w": -2 ** 64, "a": 2 ** 63}) == (None, True)
    assert M.eval_value(col("w") * col("a"), SCHEMA, {"w": 2 ** 64, "a": 2 ** 63}) == (None, True)


def test_doubles_bit_for_bit():
    e = col("x") + col("y")
    v, o = M.eval_value(e, SCHEMA, {"x": 0.1, "y": 0.2})
    assert (M.bits(v), o) == (0x3FD3333333333334, False)
    v, _ = M.eval_value(e, SCHEMA, {"x": float("nan"), "y": 1.0})
    assert math.isnan(v)
    v, _ = M.eval_value(col("x") * col("y"), SCHEMA, {"x": -0.0, "y": 5.0})
    assert M.bits(v) == 0x8000000000000000
    v, _ = M.eval_value(e, SCHEMA, {"x": -0.0, "y": 0.0})
    assert M.bits(v) == 0
    assert M.eval_value(e, SCHEMA, {"x": None, "y": 0.0}) == (None, False)
    v, o = M.eval_value(col("x") * col("y"), SCHEMA, {"x": 1e308, "y": 10.0})
    assert v == float("inf") and not o  # a double never counts as an overflow


def test_count_and_names():
    rows = [{"a": 2 ** 63 - 1, "b": 1}, {"a": 1, "b": None}, {"a": 1, "b": 2}, {"a": -2 ** 63, "b": -1}]
    assert M.eval_column(col("a") + col("b"), SCHEMA, rows) == ([None, None, 3, None], 2)
    roots = {"a", "b"}
    assert M.check_names(["r", "s"], roots) is None
    assert M.check_names(["r", ""], roots) == "empty"
    assert M.check_names(["r", "r"], roots) == "twice"
    assert M.check_names(["r", "b"], roots) == "root"
