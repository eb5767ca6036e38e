"""Predicate.in_list / not_in / between: what flatten() emits for them (the node list of include/orcgpu.h: an ORCGPU_PRED_IN leaf
with its ORCGPU_PRED_LITERAL nodes behind it) and the arguments they refuse.  No GPU, no library."""
import decimal

import pytest

from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V


def nodes(pred):
    arr, keep = pred.flatten()
    return [(n.op, n.n_children, n.column, n.value_type, n.value_is_null, n.i, n.f, n.s[:n.s_len] if n.s is not None else None) for n in arr]


def test_the_ops_are_those_of_the_header():
    assert (PR.IN, PR.LITERAL, PR.LIKE) == (17, 18, 16)


def test_in_list_is_a_leaf_with_its_literal_nodes_behind_it():
    got = nodes(P.in_list("k", [V.Int64(5), V.Int8(-1), V.Int64(None)]))
    assert got == [(PR.IN, 3, b"k", 0, 0, 0, 0.0, None),
                   (PR.LITERAL, 0, None, PR.PV_INT64, 0, 5, 0.0, None),
                   (PR.LITERAL, 0, None, PR.PV_INT8, 0, -1, 0.0, None),
                   (PR.LITERAL, 0, None, PR.PV_INT64, 1, 0, 0.0, None)]
    assert nodes(P.in_list("k", [])) == [(PR.IN, 0, b"k", 0, 0, 0, 0.0, None)]
    assert nodes(P.in_list("k", iter([V.Float32(1.5)]))) == [(PR.IN, 1, b"k", 0, 0, 0, 0.0, None), (PR.LITERAL, 0, None, PR.PV_FLOAT32, 0, 0, 1.5, None)]
    got = nodes(P.in_list("s", (V.Utf8("é"), V.Utf8(b"\xffa"), V.Utf8(""), V.Boolean(True))))
    assert [g[7] for g in got] == [None, "é".encode(), b"\xffa", b"", None] and got[4][5] == 1
    got = nodes(P.in_list("d", [V.Decimal128(decimal.Decimal("-1.50")), V.TimestampNs(7)]))
    assert got[1][3:6] == (PR.PV_DECIMAL128, 0, 2) and got[1][7] == (-150).to_bytes(16, "little", signed=True)
    assert got[2][3:6] == (PR.PV_TIMESTAMP_NS, 0, 7)


def test_not_in_and_between_are_sugar():
    assert nodes(P.not_in("k", [V.Int64(5)])) == [(PR.NOT, 1, None, 0, 0, 0, 0.0, None)] + nodes(P.in_list("k", [V.Int64(5)]))
    assert nodes(P.between("k", V.Int64(1), V.Int64(9))) == nodes(P.and_([P.gte("k", V.Int64(1)), P.lte("k", V.Int64(9))]))
    tree = P.or_([P.in_list("a", [V.Int64(1), V.Int64(2)]), P.eq("b", V.Utf8("x")), P.not_in("c", [])])
    assert [(g[0], g[1]) for g in nodes(tree)] == [(PR.OR, 3), (PR.IN, 2), (PR.LITERAL, 0), (PR.LITERAL, 0), (PR.EQ, 0), (PR.NOT, 1), (PR.IN, 0)]


def test_65536_values_flatten():
    arr, _ = P.in_list("k", [V.Int64(k) for k in range(65536)]).flatten()
    assert len(arr) == 65537 and arr[0].n_children == 65536 and arr[65536].i == 65535


@pytest.mark.parametrize("values", [5, None, V.Int64(5), "ab", b"ab", [5], [V.Int64(5), 6], [V.Int64(1), None], ["a"], [(1, 2)]])
def test_anything_but_an_iterable_of_predicate_values_is_a_type_error(values):
    with pytest.raises(TypeError):
        P.in_list("k", values)
    with pytest.raises(TypeError):
        P.not_in("k", values)
