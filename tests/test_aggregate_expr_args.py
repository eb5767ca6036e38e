"""orc_rust_amd.aggregate's expressions as arguments: col / lit, the overloaded operators, the pre-order of Expr.flatten(), the
literal encodings, every TypeError / ValueError, and that specs of names alone still give the arrays they gave before.  No library
call: nothing here loads liborcgpu.so."""
import decimal

import pytest

from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import Agg, Expr, col, lit

D = decimal.Decimal


def shape(e):
    """the tree as nested tuples"""
    if e.op == A.EXPR_COLUMN:
        return e.column
    if e.op == A.EXPR_LITERAL:
        return e.value
    return ({A.EXPR_ADD: "+", A.EXPR_SUB: "-", A.EXPR_MUL: "*", A.EXPR_NEG: "neg"}[e.op],) + tuple(shape(c) for c in e.children)


def test_operators_build_the_tree_and_wrap_plain_numbers():
    p, d = col("p"), col("d")
    assert shape(p * (1 - d)) == ("*", "p", ("-", 1, "d"))
    assert shape((p + 2) * 3 - d) == ("-", ("*", ("+", "p", 2), 3), "d")
    assert shape(2 + p) == ("+", 2, "p") and shape(2 * p) == ("*", 2, "p") and shape(2 - p) == ("-", 2, "p")
    assert shape(-p * d) == ("*", ("neg", "p"), "d")
    assert shape(p * D("1.5")) == ("*", "p", (15, 1)) and shape(0.5 * p) == ("*", 0.5, "p")
    assert isinstance(p + 1, Expr) and (p * (1 - d)).node_count() == 5
    assert repr(Agg.sum(p * (1 - d))) == "Agg.sum((col('p') * (lit(1) - col('d'))))"
    assert repr(Agg.avg("p")) == "Agg.avg('p')" and repr(Agg.sum(-p + D("0.50"))) == "Agg.sum(((-col('p')) + lit(Decimal('0.50'))))"


def test_flatten_is_pre_order_and_keeps_its_bytes():
    e = col("price") * (1 - col("disc")) * (D("1.00") + col("tax"))
    nodes, keep = e.flatten()
    assert [n.op for n in nodes] == [A.EXPR_MUL, A.EXPR_MUL, A.EXPR_COLUMN, A.EXPR_SUB, A.EXPR_LITERAL, A.EXPR_COLUMN, A.EXPR_ADD, A.EXPR_LITERAL, A.EXPR_COLUMN]
    assert [n.column for n in nodes if n.op == A.EXPR_COLUMN] == [b"price", b"disc", b"tax"]
    assert (nodes[4].value_type, nodes[4].i) == (A.PV_INT64, 1)
    assert (nodes[7].value_type, nodes[7].i, nodes[7].s_len, nodes[7].s[:2]) == (A.PV_DECIMAL128, 2, 16, b"d")       # 100 at scale 2
    assert b"price" in keep and (100).to_bytes(16, "little") in keep
    nodes, _ = (col("f") * 0.25).flatten()
    assert (nodes[2].value_type, nodes[2].f) == (A.PV_FLOAT64, 0.25)


def decimal_bytes(e):
    nodes, keep = e.flatten()
    n = nodes[0]
    raw = [b for b in keep if isinstance(b, bytes) and len(b) == 16][0]
    return int.from_bytes(raw, "little", signed=True), n.i, n.s_len


def test_literal_encodings():
    assert decimal_bytes(lit(D("-12.345"))) == (-12345, 3, 16)
    assert decimal_bytes(lit(D("1E+2"))) == (100, 0, 16)              # a positive exponent is written out at scale 0
    assert decimal_bytes(lit(D("-2.5E+3"))) == (-2500, 0, 16)
    assert decimal_bytes(lit(D("1E-38"))) == (1, 38, 16)              # scale 38
    assert decimal_bytes(lit(D("0." + "9" * 38))) == (10 ** 38 - 1, 38, 16)
    assert decimal_bytes(lit(D("-" + "9" * 38))) == (-(10 ** 38 - 1), 0, 16)
    assert decimal_bytes(lit(D("0"))) == (0, 0, 16) and decimal_bytes(lit(D("0.00"))) == (0, 2, 16)
    assert lit(-2 ** 63).value == -2 ** 63 and lit(2 ** 63 - 1).value_type == A.PV_INT64
    assert lit(1.5).value_type == A.PV_FLOAT64


def test_every_type_error_and_value_error():
    for bad in (True, False, "1", None, b"1", [1], 1j):
        with pytest.raises(TypeError):
            lit(bad)
    with pytest.raises(TypeError):
        col("p") + "1"
    with pytest.raises(TypeError):
        True * col("p")
    for bad in (D("NaN"), D("Infinity"), D("-Infinity"), D("sNaN"), D("1E+38"), D("-1E+38"), D("1" + "0" * 38), D("1E-39"), D("9" * 39), 2 ** 63, -2 ** 63 - 1):
        with pytest.raises(ValueError):
            lit(bad)
    for bad in (None, 1, b"p"):
        with pytest.raises(TypeError):
            col(bad)
    with pytest.raises(ValueError):
        col("")
    for ctor in (Agg.sum, Agg.avg):
        for bad in (None, 1, 1.5, b"p", ["p"], D("1")):
            with pytest.raises(TypeError) as e:
                ctor(bad)
            assert "a column name must be a str" in str(e.value)
        with pytest.raises(ValueError):
            ctor("")
    for ctor in (Agg.min, Agg.max, Agg.count):      # no expressions there
        with pytest.raises(TypeError):
            ctor(col("p"))


def test_ops_and_expr_array():
    assert (A.SUM_EXPR, A.AVG, A.AVG_EXPR) == (6, 7, 8)
    e = col("p") * 2
    assert (Agg.sum(e).op, Agg.avg(e).op, Agg.avg("p").op, Agg.sum("p").op) == (A.SUM_EXPR, A.AVG_EXPR, A.AVG, A.SUM)
    specs = [Agg.count_rows(), Agg.sum(e), Agg.avg("p"), Agg.avg(e + 1)]
    arr, _ = A.spec_array(specs)
    assert [(s.op, s.column, s.column2) for s in arr] == [(0, None, None), (6, None, None), (7, b"p", None), (8, None, None)]
    exprs, keep = A.expr_array(specs)
    assert [x.n_nodes for x in exprs] == [0, 3, 0, 5] and not exprs[0].nodes and not exprs[2].nodes
    assert [exprs[3].nodes[k].op for k in range(5)] == [A.EXPR_ADD, A.EXPR_MUL, A.EXPR_COLUMN, A.EXPR_LITERAL, A.EXPR_LITERAL]


def test_specs_of_names_alone_are_what_they_were():
    specs = [Agg.count_rows(), Agg.count("a"), Agg.sum("a"), Agg.min("a"), Agg.max("b"), Agg.sum_product("a", "b")]
    arr, keep = A.spec_array(specs)
    assert [(s.op, s.column, s.column2) for s in arr] == [(0, None, None), (1, b"a", None), (2, b"a", None), (3, b"a", None), (4, b"b", None), (5, b"a", b"b")]
    assert keep == [b"a", b"a", b"a", b"b", b"a", b"b"]
    assert A.expr_array(specs) == (None, [])         # the bindings then call the entry points without expressions
    assert repr(specs[5]) == "Agg.sum_product('a', 'b')" and repr(specs[0]) == "Agg.count_rows()"
