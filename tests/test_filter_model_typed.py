"""The model of the Decimal and Timestamp leaves (tests/filter_model_typed.py) against pyarrow.compute, where both are defined:
pyarrow brings the two decimals to a common scale (which must fit 38 digits) and the two timestamps to a common unit (which must
fit int64); the model compares fractions and integers of nanoseconds.  Without a GPU."""
import datetime
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import filter_model as FM
import filter_model_typed as FT
from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

D = decimal.Decimal
PC_OPS = {PR.EQ: pc.equal, PR.NE: pc.not_equal, PR.LT: pc.less, PR.LE: pc.less_equal, PR.GT: pc.greater, PR.GE: pc.greater_equal}


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(5)
    n = 300
    nulls = lambda vals: [None if rng.random() < 0.3 else v for v in vals]
    cents = [D(int(x)) / 100 for x in rng.integers(-8, 9, n)]
    nanos = [D(int(x)).scaleb(-9) for x in rng.integers(-3, 4, n) * 10 ** 9 + rng.integers(-2, 3, n)]
    ts = rng.integers(-3, 4, n) * 10 ** 9 + rng.integers(-2, 3, n) * 1000 + rng.integers(-1, 2, n)
    return pa.table({
        "d2": pa.array(nulls(cents), pa.decimal128(10, 2)),
        "d9": pa.array(nulls(nanos), pa.decimal128(18, 9)),
        "ns": pa.array(nulls(ts.tolist()), pa.timestamp("ns")),
        "us": pa.array(nulls((ts // 1000).tolist()), pa.timestamp("us")),
        "utc": pa.array(nulls((ts // 10 ** 6).tolist()), pa.timestamp("ms", tz="UTC")),
        "i": pa.array(rng.integers(0, 5, n), pa.int64()),
    })


def check(table, pred, want_true):
    """want_true: a pyarrow Boolean array, null where the comparison is UNKNOWN"""
    t, f = FT.evaluate(pred, table)
    assert t.tolist() == want_true.fill_null(False).to_pylist()
    assert f.tolist() == pc.invert(want_true).fill_null(False).to_pylist()
    assert not (t & f).any()


def test_decimal_leaves_agree_with_pyarrow(table):
    literals = [D("0.05"), D("0.055"), D("-0.05"), D("0"), D("0.1"), D("-0.0700"), D("1"), D("-2.000000001"), D("2.000000000"), D("0.08")]
    for name in ("d2", "d9"):
        for lit in literals:
            scalar = pa.scalar(lit, pa.decimal128(20, -lit.as_tuple().exponent))
            for op, fn in PC_OPS.items():
                check(table, P.comparison(name, op, V.Decimal128(lit)), fn(table.column(name), scalar))
    # the (unscaled, scale) form is the same literal
    for op in PC_OPS:
        a, b = FT.evaluate(P.comparison("d2", op, V.Decimal128((55, 3))), table), FT.evaluate(P.comparison("d2", op, V.Decimal128(D("0.055"))), table)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_timestamp_leaves_agree_with_pyarrow(table):
    for name in ("ns", "us", "utc"):
        tz = table.schema.field(name).type.tz
        for ns in (0, 1, -1, 999, 1000, 1001, -1000, -1001, 10 ** 6, 10 ** 6 + 1, -10 ** 9, -10 ** 9 - 1, 2 * 10 ** 9 + 1000, -2 * 10 ** 9 - 2000):
            scalar = pa.scalar(ns, pa.timestamp("ns", tz=tz))
            for op, fn in PC_OPS.items():
                check(table, P.comparison(name, op, V.TimestampNs(ns)), fn(table.column(name), scalar))
    # a datetime literal is the same instant
    lit = datetime.datetime(1969, 12, 31, 23, 59, 58)
    for op, fn in PC_OPS.items():
        check(table, P.comparison("us", op, V.TimestampNs(lit)), fn(table.column("us"), pa.scalar(lit, pa.timestamp("us"))))


def test_three_valued_logic_and_refusals(table):
    dec, ts, i = P.lt("d2", V.Decimal128(D("0.02"))), P.gte("ns", V.TimestampNs(0)), P.eq("i", V.Int64(1))
    d = pc.less(table.column("d2"), pa.scalar(D("0.02"), pa.decimal128(10, 2)))
    t = pc.greater_equal(table.column("ns"), pa.scalar(0, pa.timestamp("ns")))
    e = pc.equal(table.column("i"), 1)
    check(table, P.not_(dec), pc.invert(d))
    check(table, P.and_([dec, ts, i]), pc.and_kleene(pc.and_kleene(d, t), e))
    check(table, P.or_([dec, P.not_(ts), i]), pc.or_kleene(pc.or_kleene(d, pc.invert(t)), e))
    # the NULL literal: UNKNOWN everywhere, also under a NOT; NOT (dec = 0.055) keeps every non-null row and no null one
    for pred in (P.eq("d2", V.Decimal128(None)), P.not_(P.ne("ns", V.TimestampNs(None)))):
        got = FT.evaluate(pred, table)
        assert not got[0].any() and not got[1].any()
    assert FT.keep_mask(P.not_(P.eq("d2", V.Decimal128(D("0.055")))), table).tolist() == table.column("d2").is_valid().to_pylist()
    for pred, code in ((P.eq("d2", V.Int64(0)), 7), (P.lt("ns", V.Int64(0)), 7), (P.lt("ns", V.Decimal128(D(1))), 7), (P.eq("d2", V.TimestampNs(0)), 7),
                       (P.eq("i", V.Decimal128(D(1))), 6), (P.eq("i", V.TimestampNs(1)), 6)):
        with pytest.raises(FM.FilterRefused) as e:
            FT.evaluate(pred, table)
        assert e.value.code == code
