"""The aggregation's model (tests/agg_model.py) held to pyarrow.compute where that computes the same thing -- sum, min_max and
count on inputs without NaN --, and to hand-written cases where it does not: empty and all-null input, NaN, -0.0, overflow.
No GPU."""
import decimal
import math

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import agg_model as AM
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

D = decimal.Decimal


def table(n, null_frac, seed=5):
    rng = np.random.default_rng(seed + n)

    def nulls(values):
        mask = rng.random(n) < null_frac if null_frac < 1.0 else np.ones(n, bool)
        return [None if m else v for v, m in zip(values, mask)]

    return pa.table({
        "i8": pa.array(nulls(rng.integers(-128, 128, n).tolist()), pa.int8()),
        "i64": pa.array(nulls(rng.integers(-2 ** 40, 2 ** 40, n).tolist()), pa.int64()),   # (pyarrow.compute.sum wraps at int64)
        "f64": pa.array(nulls((rng.standard_normal(n) * 1e6).tolist()), pa.float64()),
        "f32": pa.array(nulls(rng.standard_normal(n).astype(np.float32).tolist()), pa.float32()),
        "dec": pa.array(nulls([D(int(x)).scaleb(-2) for x in rng.integers(-10 ** 14, 10 ** 14, n)]), pa.decimal128(15, 2)),
        "b": pa.array(nulls((rng.random(n) < 0.5).tolist()), pa.bool_()),
        "d": pa.array(nulls(rng.integers(-20000, 20000, n).tolist()), pa.date32()),
        "s": pa.array(nulls(["v%d" % x for x in range(n)]), pa.string()),
    })


@pytest.mark.parametrize("n", [1, 64, 1000])
@pytest.mark.parametrize("null_frac", [0.0, 0.3])
def test_model_against_pyarrow_compute(n, null_frac):
    t = table(n, null_frac)
    pred = P.gt("i8", V.Int8(0))
    keep = AM.kept_mask(t, pred)
    kept = t.filter(pa.array(keep))
    assert AM.aggregate(t, [Agg.count_rows()], pred) == [kept.num_rows]
    for name in t.column_names:
        assert AM.aggregate(t, [Agg.count(name)], pred) == [pc.count(kept.column(name)).as_py()], name
    for name in ("i8", "i64", "dec"):
        assert AM.aggregate(t, [Agg.sum(name)], pred) == [pc.sum(kept.column(name).cast(pa.decimal128(38, 2)) if name == "dec" else kept.column(name)).as_py()], name
    for name in ("f64", "f32"):
        got, = AM.aggregate(t, [Agg.sum(name)], pred)
        want = pc.sum(kept.column(name).cast(pa.float64())).as_py()
        xs = [x for x in kept.column(name).to_pylist() if x is not None]
        assert (got is None and want is None) or abs(got - want) <= AM.float_bound(xs), name
    for name in ("i8", "i64", "dec", "f64", "f32", "d"):
        mm = pc.min_max(kept.column(name).cast(pa.int32()) if name == "d" else kept.column(name)).as_py()
        assert AM.aggregate(t, [Agg.min(name), Agg.max(name)], pred) == [mm["min"], mm["max"]], name
    b = [x for x in kept.column("b").to_pylist() if x is not None]
    assert AM.aggregate(t, [Agg.min("b"), Agg.max("b")], pred) == ([int(min(b)), int(max(b))] if b else [None, None])


def test_empty_and_all_null():
    for t in (table(0, 0.0), table(40, 1.0)):
        specs = [Agg.count_rows(), Agg.count("i64"), Agg.sum("i64"), Agg.sum("f64"), Agg.sum("dec"), Agg.min("f64"), Agg.max("dec"), Agg.sum_product("i64", "i8"),
                 Agg.sum_product("dec", "dec"), Agg.min("b")]
        assert AM.aggregate(t, specs) == [t.num_rows, 0] + [None] * 8
    t = table(40, 0.0)
    assert AM.aggregate(t, [Agg.count_rows(), Agg.sum("i64")], P.lt("i8", V.Int8(-128))) == [0, None]   # a filter that keeps nothing


def test_nan_and_zero():
    nan, inf = math.nan, math.inf
    t = pa.table({"x": pa.array([1.0, nan, -2.0, None]), "allnan": pa.array([nan, nan, None, nan]), "inf": pa.array([inf, 1.0, -inf, None]),
                  "oneinf": pa.array([inf, 1.0, 2.0, None]), "z": pa.array([-0.0, 0.0, None, -0.0])})
    got = AM.aggregate(t, [Agg.sum("x"), Agg.min("x"), Agg.max("x"), Agg.min("allnan"), Agg.max("allnan"), Agg.sum("inf"), Agg.sum("oneinf"), Agg.min("inf"),
                           Agg.sum_product("x", "oneinf"), Agg.min("z"), Agg.max("z"), Agg.sum("z")])
    assert got[0] != got[0] and got[1:3] == [-2.0, 1.0]
    assert got[3] != got[3] and got[4] != got[4]
    assert got[5] != got[5] and got[6] == inf and got[7] == -inf
    assert got[8] != got[8]                       # 1 * inf + NaN * 1 + ...
    assert got[9] == 0.0 and got[10] == 0.0 and got[11] == 0.0
    assert AM.same(-0.0, 0.0) and AM.same(nan, nan) and not AM.same(nan, 0.0) and not AM.same(1, 1.0) and AM.same(None, None)


def test_overflow():
    big, small = 2 ** 63 - 1, -2 ** 63
    t = pa.table({"a": pa.array([small] * 3, pa.int64()), "b": pa.array([big] * 3, pa.int64()),
                  "d38": pa.array([D(10 ** 38 - 2), D(1), D(1)], pa.decimal128(38, 0)),
                  "wide": pa.array([D(2 ** 63), D(1), D(1)], pa.decimal128(38, 0)), "one": pa.array([D(1)] * 3, pa.decimal128(38, 0))})
    assert AM.aggregate(t, [Agg.sum("a"), Agg.sum("b")]) == [3 * small, 3 * big]                    # far inside int128
    assert AM.aggregate(t, [Agg.sum_product("a", "a")]) == [AM.OVERFLOW]                            # 3 * 2^126 > 2^127 - 1
    keep2 = np.array([True, True, False])
    assert AM.aggregate(t, [Agg.sum_product("a", "a")], keep=np.array([True, False, False])) == [2 ** 126]
    assert AM.aggregate(t, [Agg.sum_product("a", "a")], keep=keep2) == [AM.OVERFLOW]                # 2^127 itself
    assert AM.aggregate(t, [Agg.sum_product("a", "b")], keep=keep2) == [2 * small * big]            # -2^127 + 2^64: it fits
    assert AM.aggregate(t, [Agg.sum_product("a", "b")]) == [AM.OVERFLOW]
    assert AM.aggregate(t, [Agg.sum("d38")], keep=keep2) == [D(10 ** 38 - 1)]
    assert AM.aggregate(t, [Agg.sum("d38")]) == [AM.OVERFLOW]
    assert AM.aggregate(t, [Agg.sum_product("wide", "one")]) == [AM.OVERFLOW]                       # an operand beyond int64
    assert AM.aggregate(t, [Agg.sum_product("wide", "one")], keep=np.array([False, True, True])) == [D(2)]


def test_selection_and_filter_combine():
    t = table(300, 0.3)
    sel = [(50, True), (100, False), (70, True), (40, False)]
    keep = AM.kept_mask(t, P.is_not_null("i64"), sel, batch_size=128)
    want = np.zeros(300, bool)
    want[50:150] = want[220:260] = True
    want &= np.array(t.column("i64").is_valid().to_pylist())
    assert (keep == want).all()
