"""The Python builders of the conversions (orc_rust_amd.aggregate.cast / decimal / round_ / floor / ceil / trunc): every argument
is checked before anything reaches the GPU; the reprs; the flattened node arrays of both languages.  No GPU."""
import decimal
import math

import pytest

import orc_rust_amd
from orc_rust_amd import aggregate as A
from orc_rust_amd import predicate as P
from orc_rust_amd.aggregate import Agg, cast, ceil, col, decimal_, floor, lit, round_, trunc


def nodes(e):
    arr, _keep = e.flatten()
    return [(n.op, n.value_type, n.i) for n in arr]


def test_the_package_exports_the_builders():
    for name in ("cast", "decimal", "round_", "floor", "ceil", "trunc"):
        assert name in orc_rust_amd.__all__ and callable(getattr(orc_rust_amd, name))
    assert isinstance(orc_rust_amd.decimal(2), A.DecimalTarget)
    assert (A.EXPR_CAST, A.EXPR_ROUND, A.EXPR_FLOOR, A.EXPR_CEIL, A.EXPR_TRUNC) == (30, 31, 32, 33, 34)
    assert (P.EXPR_CAST, P.EXPR_ROUND, P.EXPR_FLOOR, P.EXPR_CEIL, P.EXPR_TRUNC) == (50, 51, 52, 53, 54)


def test_cast_builds_the_node_and_checks_its_target():
    assert nodes(cast("a", "int64")) == [(A.EXPR_CAST, A.PV_INT64, 0), (A.EXPR_COLUMN, 0, 0)]
    assert nodes(cast(col("a") + 1, "float64"))[0] == (A.EXPR_CAST, A.PV_FLOAT64, 0)
    assert nodes(cast(2.5, decimal_(38)))[:2] == [(A.EXPR_CAST, A.PV_DECIMAL128, 38), (A.EXPR_LITERAL, A.PV_FLOAT64, 0)]
    assert nodes(cast(decimal.Decimal("1.5"), decimal_(0)))[0] == (A.EXPR_CAST, A.PV_DECIMAL128, 0)
    for bad in (None, 64, 2.0, b"int64", ("decimal", 2)):
        with pytest.raises(TypeError):
            cast("a", bad)
    for bad in ("int32", "double", "decimal", "", "INT64"):
        with pytest.raises(ValueError):
            cast("a", bad)
    for bad in (True, 2.0, "2", None):
        with pytest.raises(TypeError):
            decimal_(bad)
    for bad in (-1, 39):
        with pytest.raises(ValueError):
            decimal_(bad)
    for bad in (None, True, b"a", [1]):
        with pytest.raises(TypeError):
            cast(bad, "int64")
    with pytest.raises(TypeError, match="condition"):
        cast(A._condition("t", col("a") < 5), "int64")


def test_round_floor_ceil_trunc_build_the_nodes_and_check_the_digits():
    assert nodes(round_("p", 2)) == [(A.EXPR_ROUND, 0, 2), (A.EXPR_COLUMN, 0, 0)]
    assert nodes(round_("p"))[0] == (A.EXPR_ROUND, 0, 0)
    assert [nodes(f("p"))[0][0] for f in (floor, ceil, trunc)] == [A.EXPR_FLOOR, A.EXPR_CEIL, A.EXPR_TRUNC]
    for bad in (True, 2.0, "2", None):
        with pytest.raises(TypeError):
            round_("p", bad)
    for bad in (-1, 39):
        with pytest.raises(ValueError):
            round_("p", bad)
    for f in (round_, floor, ceil, trunc):
        for bad in (None, False, b"p", {}):
            with pytest.raises(TypeError):
                f(bad)
        with pytest.raises(TypeError, match="condition"):
            f(A._condition("t", col("a") < 5))


def test_the_python_protocols_build_the_nodes():
    a = col("a")
    assert repr(round(a, 2)) == "round_(col('a'), 2)" and repr(round(a)) == "round_(col('a'), 0)"
    assert repr(math.floor(a)) == "floor(col('a'))" and repr(math.ceil(a)) == "ceil(col('a'))" and repr(math.trunc(a)) == "trunc(col('a'))"
    assert nodes(round(a, 2)) == nodes(round_("a", 2)) and nodes(math.floor(a / 7)) == nodes(floor(col("a") / 7))
    with pytest.raises(ValueError):
        round(a, -1)
    with pytest.raises(TypeError):
        round(a, 1.5)


def test_reprs():
    assert repr(cast("a", "int64")) == "cast(col('a'), 'int64')"
    assert repr(cast(col("a") * 2, "float64")) == "cast((col('a') * lit(2)), 'float64')"
    assert repr(cast("a", decimal_(4))) == "cast(col('a'), decimal(4))" and repr(decimal_(4)) == "decimal(4)"
    assert repr(Agg.sum(cast("q", "float64") * col("x"))) == "Agg.sum((cast(col('q'), 'float64') * col('x')))"
    assert repr(trunc(lit(2.5))) == "trunc(lit(2.5))"


def test_a_filter_leaf_carries_the_nodes_20_further_on():
    pred = cast(floor(col("p") / 1000), "int64") >= round_("a", 1)
    arr, _keep = pred.flatten()
    got = [(n.op, n.n_children, n.value_type, n.i) for n in arr]
    assert got[0][0] == P.CMP_EXPR and got[0][1] == 2
    assert got[1] == (P.EXPR_CAST, 1, A.PV_INT64, 0) and got[2][:2] == (P.EXPR_FLOOR, 1) and got[3][:2] == (P.EXPR_DIV, 2)
    assert got[6] == (P.EXPR_ROUND, 1, 0, 1) and got[7][0] == P.EXPR_COLUMN
    arr, _keep = (cast("x", decimal_(3)) < 5).flatten()
    assert (arr[1].op, arr[1].value_type, arr[1].i) == (P.EXPR_CAST, A.PV_DECIMAL128, 3)


def test_node_count_and_nesting():
    e = cast(round_(col("a") / 3, 2), "float64") * col("x")
    assert e.node_count() == 7 and len(nodes(e)) == 7
    assert A.when(cast("x", "int64") > 3, floor("p"), None).node_count() == 8
