"""when / case / coalesce / nullif / abs_ in Python (orc_rust_amd.aggregate): the refusals with their exception types, repr, the
flattened nodes in both numberings, and a builder that is unchanged without a new node.  No GPU, no library."""
import decimal

import pytest

import orc_rust_amd
from orc_rust_amd import aggregate as A
from orc_rust_amd import predicate as PR
from orc_rust_amd.aggregate import abs_, case, coalesce, col, lit, nullif, when
from orc_rust_amd.key_set import KeySet
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

a, b = col("a"), col("b")


def nodes(e):
    return [(n.op, n.i) for n in e.flatten()[0]]


def test_the_numbers_and_the_exports():
    assert (A.EXPR_IF, A.EXPR_COALESCE, A.EXPR_ABS, A.EXPR_NULL, A.EXPR_CMP, A.EXPR_IS_NULL, A.EXPR_AND, A.EXPR_OR, A.EXPR_NOT) == tuple(range(21, 30))
    assert (PR.EXPR_IF, PR.EXPR_COALESCE, PR.EXPR_ABS, PR.EXPR_NULL, PR.EXPR_CMP, PR.EXPR_IS_NULL, PR.EXPR_AND, PR.EXPR_OR, PR.EXPR_NOT) == tuple(range(41, 50))
    for name in ("when", "case", "coalesce", "nullif", "abs_"):
        assert getattr(orc_rust_amd, name) is getattr(A, name) and name in orc_rust_amd.__all__
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orcgpu.h")).read()
    for text in ("ORCGPU_AGG_EXPR_IF = 21", "ORCGPU_AGG_EXPR_NOT = 29", "ORCGPU_PRED_EXPR_IF = 41", "ORCGPU_PRED_EXPR_NOT = 49", "CONDITIONALS"):
        assert text in header


def test_the_flattened_nodes_in_the_aggregates_numbering():
    assert nodes(when(a < 5, b, 0)) == [(21, 0), (25, PR.LT), (0, 0), (1, 5), (0, 0), (1, 0)]
    assert nodes(when(a.ne(b), None, 1)) == [(21, 0), (25, PR.NE), (0, 0), (0, 0), (24, 0), (1, 1)]
    assert nodes(coalesce("a", 0, b)) == [(22, 0), (0, 0), (22, 0), (1, 0), (0, 0)]
    assert nodes(abs(a - b)) == nodes(abs_(a - b)) == [(23, 0), (3, 0), (0, 0), (0, 0)]
    # nullif is sugar: when(a = b, NULL, a), a's nodes twice
    assert nodes(nullif(a + 1, 0)) == [(21, 0), (25, PR.EQ), (2, 0), (0, 0), (1, 1), (1, 0), (24, 0), (2, 0), (0, 0), (1, 1)]
    assert nullif(a + 1, 0).node_count() == 10
    # case nests from the right
    assert nodes(case([(a < 10, 0), (a < 25, 1)], 2)) == nodes(when(a < 10, 0, when(a < 25, 1, 2)))
    assert nodes(case([(a < 10, 0)])) == [(21, 0), (25, PR.LT), (0, 0), (1, 10), (1, 0), (24, 0)]
    # the conditions: & | ~, is_null / is_not_null, a plain numeric comparison leaf
    cond = (P.is_not_null("a") & P.lt("a", V.Int32(5))) | ~P.gte("b", V.Decimal128(decimal.Decimal("1.50")))
    got = when(cond, 1, 0).flatten()[0]
    assert [(n.op, n.i) for n in got][:10] == [(21, 0), (28, 0), (27, 0), (29, 0), (26, 0), (0, 0), (25, PR.LT), (0, 0), (1, 5), (29, 0)]
    assert [(n.op, n.i) for n in got][10:14] == [(25, PR.GE), (0, 0), (1, 2), (1, 1)] and got[12].value_type == A.PV_DECIMAL128
    assert nodes(when(P.and_([a < 1, a < 2, a < 3]), 1, 0))[:3] == [(21, 0), (27, 0), (27, 0)]
    assert nodes(when(P.gt("a", V.Float64(0.5)), 1.0, 0.0))[3] == (1, 0) and when(P.gt("a", V.Float64(0.5)), 1.0, 0.0).flatten()[0][3].f == 0.5


def test_the_flattened_nodes_in_the_predicates_numbering():
    flat = (when(a < b, a, None) > 3).flatten()[0]
    assert [(n.op, n.i, n.n_children) for n in flat] == [(19, PR.GT, 2), (41, 0, 3), (45, PR.LT, 2), (20, 0, 0), (20, 0, 0), (20, 0, 0), (44, 0, 0), (21, 3, 0)]
    flat = (abs(a) + coalesce(a, 1)).eq(nullif(b, 0)).flatten()[0]
    assert [(n.op, n.n_children) for n in flat] == [(19, 2), (22, 2), (43, 1), (20, 0), (42, 2), (20, 0), (21, 0), (41, 3), (45, 2), (20, 0), (21, 0), (44, 0), (20, 0)]
    flat = when(P.is_null("a") | ~(a < 1), 1, 0).ne(0).flatten()[0]
    assert [n.op for n in flat][:6] == [19, 41, 48, 46, 20, 49]


def test_repr():
    assert repr(when(a < 5, b, None)) == "when((col('a') < lit(5)), col('b'), None)"
    assert repr(case([(a < 10, 0), (a < 25, 1)], 2)) == "when((col('a') < lit(10)), lit(0), when((col('a') < lit(25)), lit(1), lit(2)))"
    assert repr(coalesce("a", 0)) == "coalesce(col('a'), lit(0))" and repr(abs(a - 1)) == "abs((col('a') - lit(1)))"
    assert repr(a / nullif(b, 0)) == "(col('a') / when((col('b') = lit(0)), None, col('b')))"
    assert repr(when(P.is_null("a") | ~(a < b) & a.ne(1), 1, 0)) == "when((is_null(col('a')) | ((~(col('a') < col('b'))) & (col('a') != lit(1)))), lit(1), lit(0))"
    assert repr(A.Agg.sum(when(a > b, a - b, 0))) == "Agg.sum(when((col('a') > col('b')), (col('a') - col('b')), lit(0)))"


def test_every_refusal():
    for bad in (5, "a", None, a, True):
        with pytest.raises(TypeError, match="condition is a Predicate"):
            when(bad, 1, 0)
    ks = KeySet.__new__(KeySet)  # (no GPU here: an unsealed shell, enough for the leaf to be named)
    ks._info, ks.max_keys = None, 16
    leaves = [P.like("s", "a%"), P.in_list("a", [V.Int32(1)]), P.eq("s", V.Utf8("x")), P.eq("a", V.Boolean(True)), P.lt("t", V.TimestampNs(5)), P.eq("a", V.Int32(None)),
              P.eq("a", 5)]
    p = P(PR.IN_SET, "a")
    p.key_set = ks
    for leaf in leaves + [p]:
        for cond in (leaf, P.and_([a < 1, leaf]), P.not_(leaf)):
            with pytest.raises(TypeError, match="Agg.where") as e:
                when(cond, 1, 0)
            assert ("like" in str(e.value)) == (leaf.op == PR.LIKE)
    with pytest.raises(ValueError, match="both branches are None"):
        when(a < 1, None)
    with pytest.raises(ValueError):
        case([])
    with pytest.raises(ValueError):
        case([(a < 1, None)])
    with pytest.raises(TypeError, match="pair"):
        case([a < 1])
    with pytest.raises(ValueError, match="no operand"):
        when(P.and_([]), 1, 0)
    for fn in (lambda v: when(a < 1, v, 0), lambda v: when(a < 1, 0, v), lambda v: coalesce(a, v), lambda v: coalesce(v, 0), lambda v: nullif(v, 0), lambda v: nullif(a, v),
               lambda v: abs_(v)):
        for bad in (True, [1], b"x", object()):
            with pytest.raises(TypeError, match="an Expr, a column name"):
                fn(bad)
    for fn in (lambda: coalesce(a, None), lambda: nullif(a, None), lambda: abs_(None)):
        with pytest.raises(TypeError):
            fn()
    with pytest.raises(TypeError):
        coalesce(a)
    cond = A._condition("x", a < 1)
    for fn in (lambda: when(a < 1, cond, 0), lambda: coalesce(cond, 0), lambda: abs_(cond)):
        with pytest.raises(TypeError, match="is a condition, not a number"):
            fn()
    with pytest.raises(ValueError, match="outside int64"):
        when(a < 1, 2 ** 63, 0)
    assert (a < 1).__and__(5) is NotImplemented and (a < 1).__or__("x") is NotImplemented


def test_a_builder_without_a_new_node_is_unchanged():
    e = (a + 1) * b / 3 - A.year("d") % 100
    assert nodes(e) == [(3, 0), (17, -1), (4, 0), (2, 0), (0, 0), (1, 1), (0, 0), (1, 3), (19, 0), (16, 0), (0, 0), (1, 100)]
    assert [(n.op, n.i) for n in (a + 1 < lit(2)).flatten()[0]] == [(19, PR.LT), (22, 0), (20, 0), (21, 1), (21, 2)]
    assert repr(e) == "((((col('a') + lit(1)) * col('b')) / lit(3)) - (year(col('d')) % lit(100)))" and e.cmp is None
    assert repr(P.and_([a < 1, P.eq("b", V.Int32(2))])) == "and_([(col('a') < lit(1)), eq('b', Int32(2))])"
