"""tests/agg_expr_model.py -- the model the expression aggregates are judged by -- against cases computed by hand, and against
pyarrow.compute where pyarrow is exact (Decimal products and sums that stay inside its precision).  No GPU, no library call."""
import decimal
import fractions

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import agg_expr_model as XM
import agg_model as AM
from orc_rust_amd.aggregate import Agg, col, lit

D = decimal.Decimal


def table():
    price = [D("100.00"), D("250.50"), None, D("-7.25"), D("0.01")]
    disc = [D("0.05"), D("0.10"), D("0.00"), None, D("1.00")]
    tax = [D("0.08"), D("0.00"), D("0.02"), D("0.04"), D("0.06")]
    return pa.table({"p": pa.array(price, pa.decimal128(15, 2)), "d": pa.array(disc, pa.decimal128(15, 2)), "t": pa.array(tax, pa.decimal128(15, 2)),
                     "w": pa.array([D("1.00001"), D("2.5"), D("-3"), None, D("0")], pa.decimal128(12, 5)),
                     "i": pa.array([1, -2, None, 4, 2 ** 62], pa.int64()), "j": pa.array([3, 5, 7, None, 4], pa.int64()),
                     "f": pa.array([0.1, 0.2, None, 1e300, -0.3], pa.float64()), "g": pa.array([3.0, None, 1.0, 1e300, 0.7], pa.float32())})


ALL = np.ones(5, bool)


def test_classes_and_refusals():
    fam = {"p": "decimal", "i": "int", "f": "float", "s": "other"}
    assert XM.classify(col("i") * 2 + col("i"), fam) == XM.INT
    assert XM.classify(col("i") * col("p"), fam) == XM.DEC
    assert XM.classify(col("i") + lit(D("0.5")), fam) == XM.DEC
    assert XM.classify(col("f") * 2 + 0.5, fam) == XM.FLOAT
    for e, status in ((col("f") + col("i"), "mismatched"), (col("i") + 0.5, "mismatched"), (col("f") + lit(D("1.5")), "mismatched"), (col("s") + 1, "mismatched"),
                      (col("nope") + 1, "invalid"), (lit(1) + lit(2), "invalid"), (col("f") + (2 ** 53 + 1), "invalid")):
        with pytest.raises(XM.Refused) as r:
            XM.classify(e, fam)
        assert r.value.status == status, e
    assert XM.classify(col("f") + 2 ** 53, fam) == XM.FLOAT


def test_scale_rule():
    sc = {"p": 2, "w": 5, "a": 19, "b": 20}
    assert XM.scale_of(col("p") * (1 - col("p")), sc) == 4
    assert XM.scale_of(col("p") * (1 - col("p")) * (1 + col("p")), sc) == 6
    assert XM.scale_of(col("p") + col("w"), sc) == 5 and XM.scale_of(-col("w"), sc) == 5
    assert XM.scale_of(col("a") * col("a"), sc) == 38
    with pytest.raises(XM.Refused) as r:
        XM.scale_of(col("a") * col("b") + 1, sc)
    assert r.value.status == "unsupported"


def test_q1_expressions_by_hand_and_null_rule():
    t = table()
    e1 = col("p") * (1 - col("d"))
    # rows 0, 1, 4 have both operands: 100.00 * 0.95 + 250.50 * 0.90 + 0.01 * 0.00
    assert XM.aggregate_expr(t, Agg.sum(e1), ALL) == D("95.0000") + D("225.4500") + D("0.0000")
    e2 = e1 * (1 + col("t"))
    assert XM.aggregate_expr(t, Agg.sum(e2), ALL) == D("95.0000") * D("1.08") + D("225.4500") * D("1.00")
    assert XM.aggregate_expr(t, Agg.sum(e2), ALL).as_tuple().exponent == -6
    assert XM.aggregate_expr(t, Agg.sum(e1), np.array([0, 0, 1, 1, 0], bool)) is None       # every kept row has a NULL operand
    assert XM.aggregate_expr(t, Agg.sum(col("p") + col("w")), ALL) == D("101.00001") + D("253.00000") + D("0.01000")  # scales 2 and 5


def test_against_pyarrow_where_it_is_exact():
    t = table()
    prod = pc.multiply(t["p"], pc.subtract(pa.scalar(D("1"), pa.decimal128(1, 0)), t["d"]))
    assert XM.aggregate_expr(t, Agg.sum(col("p") * (1 - col("d"))), ALL) == pc.sum(prod).as_py()
    assert XM.aggregate_expr(t, Agg.sum(col("i") * col("j")), np.array([1, 1, 1, 1, 0], bool)) == pc.sum(pc.multiply(t["i"].slice(0, 4), t["j"].slice(0, 4))).as_py()
    assert XM.aggregate_expr(t, Agg.avg("j"), ALL) == pc.mean(t["j"]).as_py()


def test_per_row_overflow_is_sticky_and_the_row_counts():
    t = pa.table({"i": pa.array([2 ** 62, 3], pa.int64()), "j": pa.array([2 ** 62, 5], pa.int64())})
    keep = np.ones(2, bool)
    e = col("i") * col("j") * col("i")            # 2^186 in row 0
    assert XM.aggregate_expr(t, Agg.sum(e), keep) == AM.OVERFLOW
    assert XM.aggregate_expr(t, Agg.sum(e), np.array([0, 1], bool)) == 45
    assert XM.eval_row(e, XM.INT, {"i": 2 ** 62, "j": 2 ** 62}, {}) == XM.ROW_OVERFLOW
    assert XM.eval_row(col("i") * col("j") * 2, XM.INT, {"i": -2 ** 63, "j": 2 ** 63 - 1}, {}) == -2 ** 63 * (2 ** 63 - 1) * 2
    # -2^127 fits, 2^127 does not
    assert XM.eval_row(col("i") * col("j") * col("j"), XM.INT, {"i": -2 ** 63, "j": 2 ** 32}, {}) == -2 ** 127
    assert XM.eval_row(col("i") * col("j") * col("j") * -1, XM.INT, {"i": -2 ** 63, "j": 2 ** 32}, {}) == XM.ROW_OVERFLOW
    # the rescale is an operation too: 10^37 (scale 0) + w (scale 5) needs 10^42
    assert XM.eval_row(col("a") + col("w"), XM.DEC, {"a": 10 ** 37, "w": 1}, {"a": 0, "w": 5}) == XM.ROW_OVERFLOW


def test_avg_rounding():
    assert XM.avg_decimal(1, 3, 2) == (3333, 6)             # 0.01 / 3 = 0.003333
    assert XM.avg_decimal(2, 3, 2) == (6667, 6)
    assert XM.avg_decimal(-2, 3, 2) == (-6667, 6)
    assert XM.avg_decimal(1, 20000, 0) == (1, 4)            # 0.00005 -> 0.0001: the tie goes away from zero
    assert XM.avg_decimal(-1, 20000, 0) == (-1, 4)
    assert XM.avg_decimal(1, 20001, 0) == (0, 4)
    assert XM.avg_decimal(7, 2, 36) == (350, 38)            # the scale is capped at 38
    assert XM.avg_decimal(7, 2, 38) == (4, 38) and XM.avg_decimal(-7, 2, 38) == (-4, 38)
    assert XM.avg_int(2 ** 53 + 1, 1) == float(2 ** 53) and XM.avg_int(2 ** 53 + 3, 1) == float(2 ** 53 + 4)     # ties to even
    s, n = 3 * (2 ** 60) + 1, 3
    assert XM.avg_int(s, n) == float(fractions.Fraction(s, n))
    t = table()
    assert XM.aggregate_expr(t, Agg.avg("p"), ALL) == D("343.26") / 4 and XM.aggregate_expr(t, Agg.avg("p"), ALL).as_tuple().exponent == -6
    assert XM.aggregate_expr(t, Agg.avg("i"), ALL) == (1 - 2 + 4 + 2 ** 62) / 4
    assert XM.aggregate_expr(t, Agg.avg("f"), np.array([1, 1, 0, 0, 1], bool)) == AM.float_sum([0.1, 0.2, -0.3]) / 3
    assert XM.aggregate_expr(t, Agg.avg("p"), np.array([0, 0, 1, 0, 0], bool)) is None


def test_float_in_operation_order():
    t = table()
    e = col("f") * (1 - col("g"))
    terms = XM.float_terms(t, Agg.sum(e), ALL)
    assert terms == [0.1 * (1 - 3.0), 1e300 * (1 - 1e300), -0.3 * (1 - float(np.float32(0.7)))]
    assert XM.aggregate_expr(t, Agg.sum(e), ALL) == float("-inf")
    assert XM.slots(col("f") * (1 - col("g"))) == 2 and XM.slots((col("f") + col("g")) * (col("f") - col("g"))) == 3
    assert XM.slots(col("f") * (lit(1) + lit(2))) == 2
    assert XM.tokens(col("p") * (1 - col("d"))) == ["*", "c:p", "-", "i:1", "c:d"]
