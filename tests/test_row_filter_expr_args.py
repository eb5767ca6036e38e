"""Predicate.compare and the comparison operators of aggregate.Expr: what they build, what flatten() emits for them (the node list
of include/orcgpu.h: an ORCGPU_PRED_CMP_EXPR leaf with its two ORCGPU_PRED_EXPR_* subtrees behind it) and the arguments they
refuse.  No GPU, no library."""
import ctypes as C
import os
from decimal import Decimal

import pytest

from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd import predicate as PR
from orc_rust_amd.aggregate import Agg, Expr, col, lit
from orc_rust_amd.arrow_reader import ArrowReader
from orc_rust_amd.predicate import Predicate
from orc_rust_amd.predicate import PredicateValue as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_headers():
    assert PR.CMP_EXPR == 19
    assert (PR.EXPR_COLUMN, PR.EXPR_LITERAL, PR.EXPR_ADD, PR.EXPR_SUB, PR.EXPR_MUL, PR.EXPR_NEG) == (20, 21, 22, 23, 24, 25)
    assert [x + 20 for x in (A.EXPR_COLUMN, A.EXPR_LITERAL, A.EXPR_ADD, A.EXPR_SUB, A.EXPR_MUL, A.EXPR_NEG)] == list(range(20, 26))
    with open(os.path.join(ROOT, "include", "orcgpu.h")) as f:
        header = f.read()
    for text in ("ORCGPU_PRED_CMP_EXPR = 19", "ORCGPU_PRED_EXPR_COLUMN = 20", "ORCGPU_PRED_EXPR_LITERAL = 21", "ORCGPU_PRED_EXPR_ADD = 22, ORCGPU_PRED_EXPR_SUB = 23, ORCGPU_PRED_EXPR_MUL = 24",
                 "ORCGPU_PRED_EXPR_NEG = 25", "int orcgpu_reader_filter_overflow_rows(const orcgpu_reader* r, uint64_t* rows);"):
        assert text in header, text
    assert "orcgpu_reader_filter_overflow_rows" in capi.EXPORTS and hasattr(capi.load(), "orcgpu_reader_filter_overflow_rows")
    assert callable(ArrowReader.filter_overflow_rows)


def test_operators_and_methods_build_the_leaf():
    a, b = col("a"), col("b")
    for p, sign, code in ((a < b, "<", PR.LT), (a <= b, "<=", PR.LE), (a > b, ">", PR.GT), (a >= b, ">=", PR.GE), (a.eq(b), "=", PR.EQ), (a.ne(b), "!=", PR.NE)):
        assert isinstance(p, Predicate) and p.op == PR.CMP_EXPR and p.cmp == code and p.exprs == (a, b) and p.children == []
        assert repr(p) == "(col('a') %s col('b'))" % sign
        q = Predicate.compare(a, sign, b)
        assert (q.op, q.cmp, q.exprs) == (p.op, p.cmp, p.exprs)
    assert repr(col("a") < col("b")) == "(col('a') < col('b'))"
    assert repr(col("p") * (1 - col("d")) > 1000) == "((col('p') * (lit(1) - col('d'))) > lit(1000))"
    # a plain number on the left: Python mirrors the operator, the leaf says the same thing
    p = 5 < col("a")
    assert (p.cmp, repr(p)) == (PR.GT, "(col('a') > lit(5))")
    p = Decimal("1.50") >= col("a")
    assert (p.cmp, repr(p)) == (PR.LE, "(col('a') <= lit(Decimal('1.50')))")
    # the leaf goes wherever a Predicate goes
    both = Predicate.and_([col("c") < col("r"), Predicate.not_(col("s") >= col("c")), Predicate.eq("m", V.Utf8("MAIL"))])
    assert repr(both) == "and_([(col('c') < col('r')), not_((col('s') >= col('c'))), eq('m', Utf8('MAIL'))])"
    agg = Agg.sum("x").where(col("a") + 1 < col("b"))
    assert agg.filter.op == PR.CMP_EXPR


def test_numbers_are_wrapped_by_lit():
    p = Predicate.compare(1, "<", col("a"))
    assert p.exprs[0].op == A.EXPR_LITERAL and (p.exprs[0].value_type, p.exprs[0].value) == (A.PV_INT64, 1) and p.cmp == PR.LT
    p = Predicate.compare(col("a"), ">=", 2.5)
    assert (p.exprs[1].value_type, p.exprs[1].value) == (A.PV_FLOAT64, 2.5)
    p = col("a").eq(Decimal("-0.75"))
    assert (p.exprs[1].value_type, p.exprs[1].value) == (A.PV_DECIMAL128, (-75, 2))
    p = Predicate.compare(1, "=", 2)  # two literal sides are allowed: the plan folds them
    assert [e.op for e in p.exprs] == [A.EXPR_LITERAL] * 2


def test_argument_errors_come_before_the_gpu():
    a = col("a")
    for bad in ("==", "<>", "lt", "", None, PR.LT, b"<"):
        with pytest.raises(ValueError):
            Predicate.compare(a, bad, 1)
    for bad in ("b", None, True, [1], V.Int64(1), Predicate.eq("a", V.Int64(1)), b"x"):
        with pytest.raises(TypeError):
            Predicate.compare(a, "<", bad)
        with pytest.raises(TypeError):
            Predicate.compare(bad, "<", a)
        with pytest.raises(TypeError):
            a < bad
        with pytest.raises(TypeError):
            a.eq(bad)
    with pytest.raises(ValueError):
        a < 2 ** 63  # lit's own range check
    with pytest.raises(ValueError):
        a.ne(Decimal("NaN"))
    with pytest.raises(TypeError):
        Agg.sum("x").where(a)  # an Expr is no Predicate


def test_expr_equality_and_hashing_are_still_identity():
    a, b = col("a"), col("a")
    assert (a == b) is False and (a != b) is True and (a == a) is True
    assert Expr.__eq__ is object.__eq__ and Expr.__ne__ is object.__ne__ and Expr.__hash__ is object.__hash__
    assert len({a, b}) == 2 and {a: 1}[a] == 1
    assert isinstance(a == 1, bool)


def nodes(p):
    arr, keep = p.flatten()
    # (the 16 bytes of a Decimal128 hold zeros: they are read through the pointer, not as a C string)
    def raw(n):
        return C.string_at(C.c_void_p.from_buffer(n, PR.PredicateNode.s.offset).value, n.s_len) if n.s_len else None

    return [(n.op, n.n_children, n.column, n.value_type, n.value_is_null, n.i, n.f, raw(n)) for n in arr]


def test_flatten_emits_the_pre_order_node_list():
    # l_commitdate < l_receiptdate
    assert nodes(col("l_commitdate") < col("l_receiptdate")) == [
        (PR.CMP_EXPR, 2, None, 0, 0, PR.LT, 0.0, None),
        (PR.EXPR_COLUMN, 0, b"l_commitdate", 0, 0, 0, 0.0, None),
        (PR.EXPR_COLUMN, 0, b"l_receiptdate", 0, 0, 0, 0.0, None)]
    # price * (1 - disc) > Decimal('1000.5'), under a NOT beside a plain leaf
    p = Predicate.and_([Predicate.not_(col("price") * (1 - col("disc")) > Decimal("1000.5")), Predicate.lt("q", V.Int64(24))])
    assert nodes(p) == [
        (PR.AND, 2, None, 0, 0, 0, 0.0, None),
        (PR.NOT, 1, None, 0, 0, 0, 0.0, None),
        (PR.CMP_EXPR, 2, None, 0, 0, PR.GT, 0.0, None),
        (PR.EXPR_MUL, 2, None, 0, 0, 0, 0.0, None),
        (PR.EXPR_COLUMN, 0, b"price", 0, 0, 0, 0.0, None),
        (PR.EXPR_SUB, 2, None, 0, 0, 0, 0.0, None),
        (PR.EXPR_LITERAL, 0, None, PR.PV_INT64, 0, 1, 0.0, None),
        (PR.EXPR_COLUMN, 0, b"disc", 0, 0, 0, 0.0, None),
        (PR.EXPR_LITERAL, 0, None, PR.PV_DECIMAL128, 0, 1, 0.0, (10005).to_bytes(16, "little", signed=True)),
        (PR.LT, 0, b"q", PR.PV_INT64, 0, 24, 0.0, None)]
    # -x + 0.5 = y, floats
    assert nodes((-col("x") + 0.5).eq(col("y"))) == [
        (PR.CMP_EXPR, 2, None, 0, 0, PR.EQ, 0.0, None),
        (PR.EXPR_ADD, 2, None, 0, 0, 0, 0.0, None),
        (PR.EXPR_NEG, 1, None, 0, 0, 0, 0.0, None),
        (PR.EXPR_COLUMN, 0, b"x", 0, 0, 0, 0.0, None),
        (PR.EXPR_LITERAL, 0, None, PR.PV_FLOAT64, 0, 0, 0.5, None),
        (PR.EXPR_COLUMN, 0, b"y", 0, 0, 0, 0.0, None)]
    # an expression's own flatten is unchanged: the aggregates' nodes, 20 lower
    arr, _ = (col("x") + 1).flatten()
    assert [n.op for n in arr] == [A.EXPR_ADD, A.EXPR_COLUMN, A.EXPR_LITERAL]
