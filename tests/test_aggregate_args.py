"""The Python side of the aggregates (orc_rust_amd/aggregate.py, ArrowReaderBuilder.aggregate, Context.result_aggregate): every
argument is checked before anything reaches the GPU, the binding declares the three entry points, and the C records become the
Python values the documentation promises.  No GPU."""
import decimal

import pytest

from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder


def test_exports_hold_the_entry_points():
    for name in ("orcgpu_result_aggregate", "orcgpu_reader_set_aggregates", "orcgpu_reader_aggregate"):
        assert name in capi.EXPORTS
        assert hasattr(capi.load(), name)
    assert capi.ABI_VERSION == 4


def test_specs():
    assert (Agg.count_rows().op, Agg.count("a").op, Agg.sum("a").op, Agg.min("a").op, Agg.max("a").op, Agg.sum_product("a", "b").op) == (0, 1, 2, 3, 4, 5)
    s = Agg.sum_product("l_extendedprice", "l_discount")
    assert (s.column, s.column2) == ("l_extendedprice", "l_discount") and "l_discount" in repr(s)
    for bad in (None, 3, b"a", ["a"]):
        for make in (Agg.count, Agg.sum, Agg.min, Agg.max):
            with pytest.raises(TypeError):
                make(bad)
        with pytest.raises(TypeError):
            Agg.sum_product("a", bad)
        with pytest.raises(TypeError):
            Agg.sum_product(bad, "a")
    with pytest.raises(ValueError):
        Agg.sum("")


def test_spec_lists_are_checked_before_the_gpu():
    with pytest.raises(ValueError):
        A.check_specs([])
    with pytest.raises(ValueError):
        A.check_specs([Agg.count_rows()] * 65)
    assert len(A.check_specs([Agg.count_rows()] * 64)) == 64
    for bad in (None, "sum", Agg.count_rows(), {"a": 1}):
        with pytest.raises(TypeError):
            A.check_specs(bad)
    for bad in (["sum(a)"], [Agg.sum("a"), None], [("sum", "a")]):
        with pytest.raises(TypeError):
            A.check_specs(bad)
    # the builder and the context check first: neither handle is touched (there is none here)
    b = ArrowReaderBuilder(None, None)
    with pytest.raises(ValueError):
        b.aggregate([])
    with pytest.raises(TypeError):
        b.aggregate("count")
    with pytest.raises(ValueError):
        b.aggregate([Agg.count_rows()] * 65)
    ctx = capi.Context.__new__(capi.Context)
    ctx.h = None
    with pytest.raises(ValueError):
        ctx.result_aggregate(None, [], ["a"])
    with pytest.raises(TypeError):
        ctx.result_aggregate(None, [1], ["a"])


def test_spec_array():
    arr, keep = A.spec_array([Agg.count_rows(), Agg.sum("a"), Agg.sum_product("a", "bé")])
    assert len(arr) == 3
    assert (arr[0].op, arr[0].column, arr[0].column2) == (A.COUNT_ROWS, None, None)
    assert (arr[1].op, arr[1].column, arr[1].column2) == (A.SUM, b"a", None)
    assert (arr[2].op, arr[2].column, arr[2].column2) == (A.SUM_PRODUCT, b"a", "bé".encode())


def value(kind, w=(0, 0, 0), f=0.0, is_null=0, overflow=0, scale_or_unit=0):
    v = A.AggValue()
    v.kind, v.is_null, v.overflow, v.scale_or_unit, v.f = kind, is_null, overflow, scale_or_unit, f
    for k in range(3):
        v.w[k] = w[k] & (2 ** 64 - 1)
    return v


def words(x):
    return [(x >> (64 * k)) & (2 ** 64 - 1) for k in range(3)]


def test_values():
    s = Agg.sum("a")
    assert A.value_of(value(A.KIND_U64, (7, 0, 0)), Agg.count_rows()) == 7
    assert A.value_of(value(A.KIND_I128, words(-2 ** 127)), s) == -2 ** 127
    assert A.value_of(value(A.KIND_I128, words(2 ** 127 - 1)), s) == 2 ** 127 - 1
    got = A.value_of(value(A.KIND_DEC128, words(-(10 ** 38 - 1)), scale_or_unit=4), s)
    assert isinstance(got, decimal.Decimal) and got == decimal.Decimal(-(10 ** 38 - 1)).scaleb(-4, decimal.Context(prec=60))
    assert A.value_of(value(A.KIND_DEC128, words(12345), scale_or_unit=2), s) == decimal.Decimal("123.45")
    assert A.value_of(value(A.KIND_F64, f=-1.5), s) == -1.5 and isinstance(A.value_of(value(A.KIND_F64, f=2.0), s), float)
    assert A.value_of(value(A.KIND_I64, words(-3), scale_or_unit=-1), Agg.min("a")) == -3
    assert not hasattr(A.value_of(value(A.KIND_I64, words(-3), scale_or_unit=-1), Agg.min("a")), "units")
    ts = A.value_of(value(A.KIND_I64, words(-2 ** 63), scale_or_unit=2), Agg.min("t"))
    assert ts == -2 ** 63 and isinstance(ts, int) and ts.units == "us"
    assert A.value_of(value(A.KIND_I64, (5, 0, 0), scale_or_unit=3), Agg.max("t")).units == "ns"
    for kind in range(5):
        assert A.value_of(value(kind, is_null=1), s) is None
    with pytest.raises(OverflowError) as e:
        A.value_of(value(A.KIND_I128, overflow=1), Agg.sum_product("a", "b"))
    assert "sum_product('a', 'b')" in str(e.value)
