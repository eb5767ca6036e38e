"""Division in an expression, in Python (orc_rust_amd.aggregate: `/`, `//`, `%`, divide): every refusal before anything reaches
the GPU, repr, the nodes flatten writes for the aggregates' numbering and the row filter's, and a builder that is unchanged when no
division is used.  No GPU, no library."""
import decimal

import pytest

import orc_rust_amd
from orc_rust_amd import aggregate as A
from orc_rust_amd import predicate as PR
from orc_rust_amd.aggregate import Agg, col, divide, lit, year
from orc_rust_amd.arrow_reader import check_computed_columns
from orc_rust_amd.predicate import Predicate


def nodes(e):
    return [(n.op, n.i) for n in e.flatten()[0]]


def test_every_python_refusal_and_repr():
    assert (A.EXPR_DIV, A.EXPR_FLOOR_DIV, A.EXPR_MOD) == (17, 18, 19) and (PR.EXPR_DIV, PR.EXPR_FLOOR_DIV, PR.EXPR_MOD) == (37, 38, 39)
    assert orc_rust_amd.divide is divide and "divide" in orc_rust_amd.__all__
    for bad in (True, 1.0, "6", decimal.Decimal(2)):
        with pytest.raises(TypeError):
            divide("a", "b", scale=bad)
    for bad in (-1, 39, 2 ** 40):
        with pytest.raises(ValueError):
            divide("a", "b", scale=bad)
    for bad in (None, [1], True, b"a"):
        with pytest.raises(TypeError):
            divide(bad, "b")
        with pytest.raises(TypeError):
            divide("a", bad)
        with pytest.raises(TypeError):
            col("a") / bad
        with pytest.raises(TypeError):
            bad % col("a")
    with pytest.raises(ValueError):
        divide("", "b")
    with pytest.raises(ValueError):
        col("a") // 2 ** 63  # (a plain number is wrapped with lit, and keeps its refusals)
    assert repr(col("a") / col("b")) == "(col('a') / col('b'))"
    assert repr(col("a") // 7) == "(col('a') // lit(7))" and repr(16 % col("a")) == "(lit(16) % col('a'))"
    assert repr(1 / col("a")) == "(lit(1) / col('a'))" and repr(2 // col("a")) == "(lit(2) // col('a'))"
    assert repr(divide("a", 3, scale=0)) == "divide(col('a'), lit(3), scale=0)" and repr(divide(col("a") + 1, "b")) == "((col('a') + lit(1)) / col('b'))"
    assert repr(year("d") % 100) == "(year(col('d')) % lit(100))"
    assert repr(col("p") / decimal.Decimal("1.5")) == "(col('p') / lit(Decimal('1.5')))" and repr(col("x") / 2.0) == "(col('x') / lit(2.0))"
    assert (col("a") / 2).node_count() == 3 and divide("a", "b").scale is None and divide("a", "b", scale=38).scale == 38


def test_the_flattened_nodes_in_both_numberings():
    # the aggregates' numbering: the scale, or -1, in the division's `i`
    assert nodes(col("a") / col("b")) == [(17, -1), (0, 0), (0, 0)]
    assert nodes(divide("a", "b", scale=0)) == [(17, 0), (0, 0), (0, 0)] and nodes(divide("a", 5, scale=38)) == [(17, 38), (0, 0), (1, 5)]
    assert nodes(col("a") // 7) == [(18, 0), (0, 0), (1, 7)] and nodes(16 % col("a")) == [(19, 0), (1, 16), (0, 0)]
    assert nodes(divide("a", "b", scale=3) % 4 + 1) == [(2, 0), (19, 0), (17, 3), (0, 0), (0, 0), (1, 4), (1, 1)]
    # the row filter's: twenty further on, the same `i`, the child counts written
    flat = (divide("a", "b", scale=7) < 3).flatten()[0]
    assert [(n.op, n.i, n.n_children) for n in flat] == [(19, PR.LT, 2), (37, 7, 2), (20, 0, 0), (20, 0, 0), (21, 3, 0)]
    flat = Predicate.compare(col("a") // 7, "=", col("b") % 16 / 2).flatten()[0]
    assert [(n.op, n.i, n.n_children) for n in flat] == [(19, PR.EQ, 2), (38, 0, 2), (20, 0, 0), (21, 7, 0), (37, -1, 2), (39, 0, 2), (20, 0, 0), (21, 16, 0), (21, 2, 0)]
    # an Agg carries its expression unchanged
    spec = Agg.sum(col("p") / col("a"))
    assert spec.expr.op == A.EXPR_DIV and nodes(spec.expr)[0] == (17, -1)
    assert check_computed_columns({"u": col("p") / col("a"), "w": col("d") // 7})[1][1].op == A.EXPR_FLOOR_DIV


def test_nothing_changes_where_no_division_is_used():
    e = col("a") * (1 - col("b")) + year("d")
    assert nodes(e) == [(2, 0), (4, 0), (0, 0), (3, 0), (1, 1), (0, 0), (16, 0), (0, 0)]
    assert repr(e) == "((col('a') * (lit(1) - col('b'))) + year(col('d')))"
    assert [(n.op, n.i) for n in (col("a") + 1 < lit(2)).flatten()[0]] == [(19, PR.LT), (22, 0), (20, 0), (21, 1), (21, 2)]
    assert col("a").scale is None and lit(1).scale is None
