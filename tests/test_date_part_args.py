"""year() .. extract() of orc_rust_amd.aggregate: what Python refuses before anything reaches the library, the repr, the flattened
nodes for the aggregates and for the row filter, and the builders that stay as they were without a date part.  No GPU."""
import pytest

import orc_rust_amd
from orc_rust_amd import aggregate as A
from orc_rust_amd import predicate as P
from orc_rust_amd.aggregate import Agg, Expr, col, day, day_of_week, day_of_year, extract, lit, month, quarter, year
from orc_rust_amd.arrow_reader import check_computed_columns

FUNCS = (year, quarter, month, day, day_of_week, day_of_year)


def test_the_constants_are_the_headers():
    assert A.EXPR_DATE_PART == 16 and P.EXPR_DATE_PART == 36 == A.EXPR_DATE_PART + P.EXPR_COLUMN
    assert A.DATE_PARTS == ("year", "quarter", "month", "day", "day_of_week", "day_of_year")
    for name in A.DATE_PARTS + ("extract",):
        assert getattr(orc_rust_amd, name) is getattr(A, name) and name in orc_rust_amd.__all__


def test_each_function_is_extract_with_its_part():
    for k, f in enumerate(FUNCS):
        e = f("d")
        assert isinstance(e, Expr) and e.op == A.EXPR_DATE_PART and e.part == k and len(e.children) == 1
        assert e.children[0].op == A.EXPR_COLUMN and e.children[0].column == "d"
        x = extract(A.DATE_PARTS[k], col("d") + 1)
        assert x.part == k and x.children[0].op == A.EXPR_ADD and repr(x) == "%s((col('d') + lit(1)))" % A.DATE_PARTS[k]


def test_refusals_in_python():
    for bad in (1, None, 1.5, b"d", lit):
        with pytest.raises(TypeError):
            year(bad)
        with pytest.raises(TypeError):
            extract("year", bad)
    with pytest.raises(ValueError):
        year("")
    for bad in ("week", "YEAR", "", "years"):
        with pytest.raises(ValueError):
            extract(bad, "d")
    for bad in (0, None, year, b"year"):
        with pytest.raises(TypeError):
            extract(bad, "d")


def test_repr_and_node_count():
    e = year("d") * 100 + month("d")
    assert repr(e) == "((year(col('d')) * lit(100)) + month(col('d')))" and e.node_count() == 7
    assert repr(-day_of_week(col("d") - col("a"))) == "(-day_of_week((col('d') - col('a'))))"
    assert repr(year("d").eq(1995)) == "(year(col('d')) = lit(1995))"
    assert repr(Agg.sum(year("d"))) == "Agg.sum(year(col('d')))"


def test_the_flattened_nodes():
    nodes, _ = (year(col("d") + 7) * 100 + day_of_year("d")).flatten()
    assert [(n.op, n.i) for n in nodes] == [(A.EXPR_ADD, 0), (A.EXPR_MUL, 0), (16, 0), (A.EXPR_ADD, 0), (A.EXPR_COLUMN, 0), (A.EXPR_LITERAL, 7),
                                            (A.EXPR_LITERAL, 100), (16, 5), (A.EXPR_COLUMN, 0)]
    assert [n.column for n in nodes if n.op == A.EXPR_COLUMN] == [b"d", b"d"]
    pn, _ = (month("d") < quarter("d") * 3).flatten()
    assert [(n.op, n.n_children, n.i) for n in pn] == [(P.CMP_EXPR, 2, P.LT), (36, 1, 2), (P.EXPR_COLUMN, 0, 0), (P.EXPR_MUL, 2, 0), (36, 1, 1), (P.EXPR_COLUMN, 0, 0),
                                                       (P.EXPR_LITERAL, 0, 3)]


def test_the_checkers_accept_the_node():
    assert check_computed_columns({"y": year("d"), "ym": year("d") * 100 + month("d")})[0][0] == "y"
    specs = [Agg.sum(year("d")), Agg.avg(day_of_year("d")), Agg.count_rows().where(year("d").eq(1995))]
    arr, _ = A.expr_array(specs)
    assert arr[0].n_nodes == 2 and arr[1].n_nodes == 2 and arr[2].n_nodes == 0 and arr[0].nodes[0].op == 16 and arr[1].nodes[0].i == 5
    farr, _ = A.filter_array(specs)
    assert farr[2].n_nodes == 4 and farr[2].nodes[1].op == 36
    deep = col("a")
    for _ in range(16):
        deep = deep + col("a")
    with pytest.raises(ValueError):
        check_computed_columns({"r": year(deep)})  # 34 nodes


def test_a_builder_without_a_date_part_is_unchanged():
    e = col("p") * (1 - col("q"))
    nodes, _ = e.flatten()
    assert [(n.op, n.i) for n in nodes] == [(A.EXPR_MUL, 0), (A.EXPR_COLUMN, 0), (A.EXPR_SUB, 0), (A.EXPR_LITERAL, 1), (A.EXPR_COLUMN, 0)]
    assert repr(e) == "(col('p') * (lit(1) - col('q')))" and e.part is None and col("p").part is None and lit(3).part is None
    pn, _ = (col("a") + 1 < col("b")).flatten()
    assert [(n.op, n.n_children, n.i) for n in pn] == [(P.CMP_EXPR, 2, P.LT), (P.EXPR_ADD, 2, 0), (P.EXPR_COLUMN, 0, 0), (P.EXPR_LITERAL, 0, 1), (P.EXPR_COLUMN, 0, 0)]
