"""Agg.where -- agg(x) FILTER (WHERE predicate) -- on the Python side: the type checks, the refusal of a second condition, repr,
and the ctypes array the bindings hand to the orcgpu_*_filters entry points (aggregate.filter_array).  No GPU."""
import ctypes as C
import gc

import pytest

from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.predicate import Predicate as P, PredicateNode, PredicateValue as V
from orc_rust_amd import predicate as PR


def test_where_returns_a_new_agg_and_leaves_the_old_one():
    p = P.like("p_type", "PROMO%")
    plain = Agg.sum(col("l_extendedprice") * (1 - col("l_discount")))
    promo = plain.where(p)
    assert promo is not plain and plain.filter is None and promo.filter is p
    assert (promo.op, promo.column, promo.column2, promo.expr) == (plain.op, plain.column, plain.column2, plain.expr)
    for a in (Agg.count_rows(), Agg.count("c"), Agg.sum("c"), Agg.avg("c"), Agg.min("c"), Agg.max("c"), Agg.sum_product("a", "b"), Agg.avg(col("c") + 1)):
        w = a.where(p)
        assert isinstance(w, Agg) and w.filter is p and a.filter is None and w.op == a.op


def test_where_type_checks():
    for bad in (None, "l_quantity > 5", 1, V.Int64(1), [P.is_null("c")], Agg.count_rows()):
        with pytest.raises(TypeError) as e:
            Agg.count_rows().where(bad)
        assert "Predicate" in str(e.value)


def test_a_second_where_is_refused_and_points_at_and_():
    once = Agg.sum("c").where(P.gt("c", V.Int64(0)))
    with pytest.raises(ValueError) as e:
        once.where(P.lt("c", V.Int64(9)))
    assert "Predicate.and_" in str(e.value) and "sum('c')" in str(e.value)
    both = Agg.sum("c").where(P.and_([P.gt("c", V.Int64(0)), P.lt("c", V.Int64(9))]))      # what the message tells the caller to write
    assert both.filter.op == PR.AND and len(both.filter.children) == 2


def test_repr_shows_the_condition():
    assert repr(Agg.count_rows()) == "Agg.count_rows()"
    assert repr(Agg.count_rows().where(P.in_list("o_orderpriority", [V.Utf8("1-URGENT"), V.Utf8("2-HIGH")]))) == \
        "Agg.count_rows().where(in_list('o_orderpriority', [Utf8('1-URGENT'), Utf8('2-HIGH')]))"
    assert repr(Agg.sum("c").where(P.not_(P.like("s", "a%", escape="\\")))) == "Agg.sum('c').where(not_(like('s', 'a%', escape='\\\\')))"
    text = repr(Agg.avg(col("a") * 2).where(P.and_([P.gte("d", V.Float64(0.5)), P.is_null("e")])))
    assert text == "Agg.avg((col('a') * lit(2))).where(and_([gte('d', Float64(0.5)), is_null('e')]))"
    # an overflow names the spec with its condition
    v = A.AggValue()
    v.overflow = 1
    with pytest.raises(OverflowError) as e:
        A.value_of(v, Agg.sum("c").where(P.gt("c", V.Int64(0))))
    assert "Agg.sum('c').where(gt('c', Int64(0)))" in str(e.value)


def test_filter_array_without_conditions_is_none():
    assert A.filter_array([Agg.count_rows(), Agg.sum("c"), Agg.sum(col("c") + 1)]) == (None, [])
    with pytest.raises(ValueError):
        A.filter_array([])
    with pytest.raises(TypeError):
        A.filter_array([P.is_null("c")])


def test_filter_array_layout_and_lifetime():
    assert A.AggFilter._fields_[0][0] == "nodes" and A.AggFilter._fields_[1][0] == "n_nodes"
    assert C.sizeof(A.AggFilter) == 16 and A.AggFilter.n_nodes.offset == 8           # {const orcgpu_predicate_node*; uint32_t}
    p = P.and_([P.like("p_type", "PROMO%"), P.in_list("g", [V.Int64(3), V.Int64(None)])])
    specs = [Agg.count_rows(), Agg.sum("x").where(p), Agg.max("y"), Agg.count("x").where(P.is_null("z"))]
    arr, keep = A.filter_array(specs)
    assert len(arr) == len(specs) == len(A.spec_array(specs)[0])                      # parallel to the specs
    assert [f.n_nodes for f in arr] == [0, 5, 0, 1]
    assert not arr[0].nodes and not arr[2].nodes                                      # {NULL, 0}: no condition
    del specs, p
    gc.collect()                                                                      # `keep` alone holds nodes, names and literal bytes
    nodes = arr[1].nodes
    assert [nodes[k].op for k in range(5)] == [PR.AND, PR.LIKE, PR.IN, PR.LITERAL, PR.LITERAL]
    assert nodes[0].n_children == 2 and nodes[2].n_children == 2
    assert nodes[1].column == b"p_type" and C.string_at(nodes[1].s, nodes[1].s_len) == b"PROMO%"
    assert nodes[2].column == b"g" and (nodes[3].i, nodes[3].value_is_null, nodes[4].value_is_null) == (3, 0, 1)
    assert arr[3].nodes[0].op == PR.IS_NULL and arr[3].nodes[0].column == b"z"
    assert C.sizeof(nodes[0]) == C.sizeof(PredicateNode)
    assert len(keep) == 2


def test_check_specs_still_accepts_conditioned_specs():
    specs = [Agg.count_rows().where(P.is_null("c")), Agg.sum("c")]
    assert A.check_specs(specs) == specs and A.check_specs(tuple(specs)) == specs
    arr, _ = A.spec_array(specs)
    assert [s.op for s in arr] == [A.COUNT_ROWS, A.SUM]
    many = [Agg.count_rows().where(P.is_null("c"))] * 65
    with pytest.raises(ValueError):
        A.check_specs(many)
