"""tests/cond_model.py against judges that are not this project's: Python's sqlite3 for CASE / COALESCE / NULLIF / ABS and the
three-valued AND / OR / NOT over small integers with NULLs; numpy.where / numpy.fabs bit for bit on doubles with NaN, both
infinities and -0.0; and the guard cases, which no judge has (SQL engines do not track an overflow per operand), by hand."""
import itertools
import sqlite3
import struct

import numpy as np
import pytest

import cond_model as M
from orc_rust_amd.aggregate import abs_, case, coalesce, col, nullif, when
from orc_rust_amd.predicate import Predicate as P

SCHEMA = {"a": "int", "b": "int", "c": "int", "p": ("dec", 2), "q": ("dec", 4), "x": "float", "y": "float"}
a, b, c, p, q, x, y = (col(n) for n in "abcpqxy")
VALS = (None, -3, 0, 2, 7)
BIG = 2 ** 63 - 1
square = a * a * a * a


def value(e, **row):
    return M.computed_value(e, SCHEMA, {k: row.get(k) for k in SCHEMA})


@pytest.fixture(scope="module")
def db():
    con = sqlite3.connect(":memory:")
    yield con
    con.close()


# (the expression, the same in SQL)
SQL = [
    (when(a < b, a, b), "CASE WHEN a < b THEN a ELSE b END"),
    (when(a.eq(b), 1, None), "CASE WHEN a = b THEN 1 END"),
    (case([(a < 0, 0), (a < 5, 1)], 2), "CASE WHEN a < 0 THEN 0 WHEN a < 5 THEN 1 ELSE 2 END"),
    (coalesce(a, b, c), "COALESCE(a, b, c)"),
    (coalesce(a, 0) + coalesce(b, 1), "COALESCE(a, 0) + COALESCE(b, 1)"),
    (nullif(a, b), "NULLIF(a, b)"),
    (abs(a - b), "ABS(a - b)"),
    (abs_(nullif(a, 2)) * 3, "ABS(NULLIF(a, 2)) * 3"),
    (when((a < b) & (b < c), 1, 0), "CASE WHEN a < b AND b < c THEN 1 ELSE 0 END"),
    (when((a < b) | (b < c), 1, 0), "CASE WHEN a < b OR b < c THEN 1 ELSE 0 END"),
    (when(~((a < b) | (b.ne(c))), 1, 0), "CASE WHEN NOT (a < b OR b <> c) THEN 1 ELSE 0 END"),
    (when(~(a <= b) & ~(c >= b), 1, 0), "CASE WHEN NOT a <= b AND NOT c >= b THEN 1 ELSE 0 END"),
    (when(P.is_null("a") | (a > c), b, None), "CASE WHEN a IS NULL OR a > c THEN b END"),
    (when(P.is_not_null("a") & P.is_null("b"), a, c), "CASE WHEN a IS NOT NULL AND b IS NULL THEN a ELSE c END"),
    (when(b.ne(0), a // abs(b), 0), "CASE WHEN b <> 0 THEN CAST(floor(CAST(a AS REAL) / ABS(b)) AS INTEGER) ELSE 0 END"),
]


@pytest.mark.parametrize("e, sql", SQL, ids=[s for _, s in SQL])
def test_sqlite_is_the_judge_over_small_integers_with_nulls(db, e, sql):
    for va, vb, vc in itertools.product(VALS, repeat=3):
        want = db.execute("SELECT %s FROM (SELECT ? AS a, ? AS b, ? AS c)" % sql, (va, vb, vc)).fetchone()[0]
        assert value(e, a=va, b=vb, c=vc) == (want, False), (sql, va, vb, vc)


def test_the_three_valued_conditions_are_sqlites(db):
    truth = {None: None, True: 1, False: 0}
    for va, vb, vc in itertools.product(VALS, repeat=3):
        row = {"a": va, "b": vb, "c": vc, "p": None, "q": None, "x": None, "y": None}
        for cond, sql in (((a < b) & (b < c), "a < b AND b < c"), ((a < b) | (b < c), "a < b OR b < c"), (~(a < b), "NOT a < b"), (a.eq(b) | ~(a.eq(b)), "a = b OR NOT a = b")):
            from orc_rust_amd.aggregate import _condition
            got = M.evaluate(_condition("t", cond), SCHEMA, row, False)
            assert truth[got] == db.execute("SELECT %s FROM (SELECT ? AS a, ? AS b, ? AS c)" % sql, (va, vb, vc)).fetchone()[0], (sql, row)


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def test_numpy_is_the_judge_on_doubles_bit_for_bit():
    nan2 = struct.unpack("<d", struct.pack("<Q", 0xfff8000000001234))[0]  # a NaN with a sign and a payload
    specials = [0.0, -0.0, 1.0, -2.5, 5e-324, 1e308, float("inf"), float("-inf"), float("nan"), nan2]
    xs = np.array([u for u in specials for _ in specials], dtype=np.float64)
    ys = np.array([v for _ in specials for v in specials], dtype=np.float64)
    with np.errstate(all="ignore"):
        judges = [(when(x < y, x, y), np.where(xs < ys, xs, ys)), (when(x >= y, x, y), np.where(xs >= ys, xs, ys)), (when(x.ne(y), x, y), np.where(xs != ys, xs, ys)),
                  (when(x.eq(y), 1.0, 0.0), np.where(xs == ys, 1.0, 0.0)), (abs(x), np.fabs(xs)), (when(x > 0.0, abs(y), -abs(y)), np.where(xs > 0.0, np.fabs(ys), -np.fabs(ys))),
                  (when(~(x < y), x, y), np.where(~(xs < ys), xs, ys))]
    for e, want in judges:
        for k in range(len(xs)):
            got, over = value(e, x=float(xs[k]), y=float(ys[k]))
            assert not over and bits(got) == bits(want[k]), (e, xs[k], ys[k])
    assert value(coalesce(x, y), x=None, y=-0.0)[0] == 0.0 and bits(value(coalesce(x, y), x=None, y=-0.0)[0]) == bits(-0.0)
    assert value(when(x < y, x, y), x=None, y=2.0) == (2.0, False) and value(when(x < y, None, y), x=1.0, y=2.0) == (None, False)
    assert value(coalesce(x / y, -1.0), x=None, y=0.0) == (-1.0, False) and value(coalesce(x / y, -1.0), x=1.0, y=0.0) == (float("inf"), False)


def test_the_guard_cases():
    # a division by zero in the untaken branch, behind a FALSE AND, behind a TRUE OR -- on either side
    assert value(when(b.ne(0), a // b, 0), a=7, b=0) == (0, False) and value(a // b, a=7, b=0) == (None, True)
    assert value(when(b.ne(0) & (a // b > 2), 1, 0), a=7, b=0) == (0, False) and value(when((a // b > 2) & b.ne(0), 1, 0), a=7, b=0) == (0, False)
    assert value(when(b.eq(0) | (a // b > 2), 1, 0), a=7, b=0) == (1, False) and value(when((a // b > 2) | b.eq(0), 1, 0), a=7, b=0) == (1, False)
    # ... and where nothing decides, overflow comes before UNKNOWN
    assert value(when((a // b > 2) & (c > 0), 1, 0), a=7, b=0, c=1) == (None, True) and value(when((a // b > 2) & (c > 0), 1, 0), a=7, b=0, c=None) == (None, True)
    assert value(when((a // b > 2) | (c > 0), 1, 0), a=7, b=0, c=0) == (None, True) and value(when((a // b > 2) & (c > 0), 1, 0), a=7, b=0, c=0) == (0, False)
    # an overflow in the taken branch, in the condition, and under NOT
    assert value(when(b > 0, square, 0), a=BIG, b=1) == (None, True) and value(when(b > 0, square, 0), a=BIG, b=0) == (0, False)
    assert value(when(square > 0, 1, 2), a=BIG) == (None, True) and value(when(~(square > 0), 1, 2), a=BIG) == (None, True)
    # NULL against overflow in arithmetic: NULL first; in IS_NULL and COALESCE the overflow shows
    assert value(square + b, a=BIG, b=None) == (None, False) and value(square + b, a=BIG, b=1) == (None, True)
    assert value(coalesce(square, 0), a=BIG) == (None, True) and value(coalesce(square, 0), a=None) == (0, False)
    # the scale alignment overflows its own branch only
    assert value(when(b > 0, a * a, p), a=BIG, b=0, p=5) == (5, False) and value(when(b > 0, a * a, p), a=BIG, b=1, p=5) == (None, True)
    assert value(when(p < q, p, q), p=125, q=12499) == (12499, False) and M.computed_type(when(p < q, p, None), SCHEMA) == ("decimal128", 2)
    assert value(abs(-(a * a * 2)), a=2 ** 63) == (None, True) and value(abs(-(a * a)), a=2 ** 63 - 1) == (None, True)  # -2^127; past Int64
    assert value(a / nullif(b, 0), a=7, b=0) == (None, False) and value(a / nullif(b, 0), a=7, b=2) == (3500000, False)


def test_the_refusals():
    from orc_rust_amd.aggregate import EXPR_CMP, EXPR_IF, EXPR_NULL, Expr
    import agg_expr_model as AEM
    for bad in (Expr(EXPR_CMP, (a, b), cmp=2), Expr(EXPR_IF, (a, b, c)), a + Expr(EXPR_NULL), Expr(EXPR_IF, (Expr(EXPR_CMP, (a, b), cmp=2), Expr(EXPR_NULL), Expr(EXPR_NULL)))):
        with pytest.raises(AEM.Refused) as e:
            M.computed_type(bad, SCHEMA)
        assert e.value.status == "invalid"
    with pytest.raises(AEM.Refused) as e:
        M.computed_type(when(a > 0, x, y), SCHEMA)
    assert e.value.status == "mismatched"
