"""The model of the IN leaf (tests/in_model.py) against a hand-written table of the SQL corners that include/orcgpu.h lists for
ORCGPU_PRED_IN, and its two ways of answering -- the OR of the EQ leaves, and a set of exact keys -- against each other.  No GPU."""
import datetime
import decimal

import numpy as np
import pyarrow as pa
import pytest

import filter_model as FM
import in_model as IM
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

T, F, U = "T", "F", "U"
NAN = float("nan")


def truth(pair):
    t, f = pair
    assert not (t & f).any()
    return [T if a else F if b else U for a, b in zip(t, f)]


def table():
    D = decimal.Decimal
    return pa.table({
        "i": pa.array([1, 2, None, -1, 0, -2 ** 63, 2 ** 63 - 1], pa.int64()),
        "f": pa.array([0.0, -0.0, None, NAN, 1.5, float("inf"), 0.1], pa.float64()),
        "g": pa.array([0.0, -0.0, None, NAN, 1.5, float("inf"), 0.1], pa.float32()),
        "b": pa.array([True, False, None, True, False, True, False], pa.bool_()),
        "s": pa.array(["", "a", None, "ab", "é", "a\x00", "b"], pa.string()),
        "d": pa.array([D("1.50"), D("-1.50"), None, D("0.00"), D("2.00"), D("0.01"), D("10.00")], pa.decimal128(10, 2)),
        "t": pa.array([0, 1000, None, -1000, 1, 2000, 5], pa.timestamp("us")),
    })


# (predicate, what every row is: the rows of table() in order)
CORNERS = [
    # a null row is UNKNOWN; a match TRUE, a non-match FALSE
    (P.in_list("i", [V.Int64(1), V.Int64(-1)]), [T, F, U, T, F, F, F]),
    # the empty list is FALSE for every row, null rows included
    (P.in_list("i", []), [F] * 7),
    (P.not_in("i", []), [T] * 7),
    # a NULL literal turns every non-match into UNKNOWN: NOT IN keeps nothing
    (P.in_list("i", [V.Int64(1), V.Int64(None)]), [T, U, U, U, U, U, U]),
    (P.not_in("i", [V.Int64(1), V.Int64(None)]), [F, U, U, U, U, U, U]),
    # nothing but NULLs: UNKNOWN everywhere
    (P.in_list("i", [V.Int64(None), V.Int32(None)]), [U] * 7),
    (P.not_in("i", [V.Int64(None)]), [U] * 7),
    # duplicates are harmless, literal kinds may be mixed, every int64 is a key
    (P.in_list("i", [V.Int8(1), V.Int64(1), V.Int16(1), V.Int32(2), V.Int64(2)]), [T, T, U, F, F, F, F]),
    (P.in_list("i", [V.Int64(-2 ** 63), V.Int64(0), V.Int64(-1), V.Int64(2 ** 63 - 1)]), [F, F, U, T, T, T, T]),
    (P.not_in("i", [V.Int64(1), V.Int64(2)]), [F, F, U, T, T, T, T]),
    # floats compare as double: a NaN literal equals no row, -0.0 and 0.0 are one key
    (P.in_list("f", [V.Float64(NAN)]), [F, F, U, F, F, F, F]),
    (P.in_list("f", [V.Float64(NAN), V.Float64(None)]), [U] * 7),
    (P.in_list("f", [V.Float64(-0.0)]), [T, T, U, F, F, F, F]),
    (P.in_list("f", [V.Float64(0.0), V.Float64(float("inf")), V.Float64(NAN)]), [T, T, U, F, F, T, F]),
    # a Float32 literal is rounded through float first: 0.1f is not the double 0.1, but it is the Float column's 0.1
    (P.in_list("f", [V.Float32(0.1), V.Float32(1.5)]), [F, F, U, F, T, F, F]),
    (P.in_list("g", [V.Float32(0.1), V.Float64(1.5)]), [F, F, U, F, T, F, T]),
    (P.in_list("g", [V.Float64(0.1)]), [F, F, U, F, F, F, F]),
    # Boolean
    (P.in_list("b", [V.Boolean(True), V.Boolean(False)]), [T, T, U, T, T, T, T]),
    (P.not_in("b", [V.Boolean(True), V.Boolean(False)]), [F, F, U, F, F, F, F]),
    (P.in_list("b", [V.Boolean(False), V.Boolean(None)]), [U, T, U, U, T, U, T]),
    # strings by their bytes, the empty one included
    (P.in_list("s", [V.Utf8(""), V.Utf8("é"), V.Utf8(b"a\x00"), V.Utf8("zz")]), [T, F, U, F, T, T, F]),
    # Decimal: a literal at another scale that matches, one that lands on no value of the scale (FALSE for valid rows, no error)
    (P.in_list("d", [V.Decimal128((15, 1)), V.Decimal128((2, 0)), V.Decimal128((1, 2))]), [T, F, U, F, T, T, F]),
    (P.in_list("d", [V.Decimal128((1505, 3))]), [F, F, U, F, F, F, F]),
    (P.in_list("d", [V.Decimal128((1505, 3)), V.Decimal128(decimal.Decimal("-1.5"))]), [F, T, U, F, F, F, F]),
    (P.not_in("d", [V.Decimal128((1505, 3))]), [T, T, U, T, T, T, T]),
    # Timestamp (microseconds): a literal between two values of the unit equals no row
    (P.in_list("t", [V.TimestampNs(1000000), V.TimestampNs(1000), V.TimestampNs(-1000000)]), [F, T, U, T, T, F, F]),
    (P.in_list("t", [V.TimestampNs(1500)]), [F, F, U, F, F, F, F]),
    (P.in_list("t", [V.TimestampNs(1500), V.TimestampNs(datetime.datetime(1970, 1, 1, 0, 0, 0, 2000))]), [F, F, U, F, F, T, F]),
    # inside a tree
    (P.and_([P.in_list("i", [V.Int64(1), V.Int64(0)]), P.not_in("s", [V.Utf8("")])]), [F, F, U, F, T, F, F]),
    (P.or_([P.in_list("i", [V.Int64(None)]), P.in_list("b", [V.Boolean(True)])]), [T, U, U, T, U, T, U]),
    (P.between("i", V.Int64(0), V.Int64(2)), [T, T, U, F, T, F, F]),
]


def test_the_corners_by_hand():
    tab = table()
    for pred, want in CORNERS:
        assert truth(IM.evaluate(pred, tab)) == want, (pred.op, pred.column, want)


def test_the_set_answers_what_the_or_of_eq_answers():
    tab = table()
    for pred, want in CORNERS:
        assert truth(IM.evaluate(pred, tab, leaf=IM.in_leaf_by_set)) == want
        assert truth(IM.evaluate(IM.or_of_eq(pred), tab)) == want
    # ... and on the shared table of the filter's tests, with lists drawn from the columns and from outside
    big = FM.make_table(600)
    rng = np.random.default_rng(3)
    for name in FM.COMPARABLE:
        pool = [v for v in big.column(name).to_pylist() if v is not None]
        for size in (0, 1, 3, 16):
            vals = [FM.literal_for(big, name, pool[rng.integers(0, len(pool))] if pool and rng.random() < 0.7 else None) for _ in range(size)]
            pred = P.in_list(name, vals)
            a, b = IM.in_leaf(pred, big), IM.in_leaf_by_set(pred, big)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), (name, size)


def test_refusals_are_those_of_eq():
    tab = table()
    for leaf in (IM.in_leaf, IM.in_leaf_by_set):
        for pred, code in ((P.in_list("i", [V.Int64(1), V.Utf8("a")]), 6), (P.in_list("s", [V.Int64(1)]), 6), (P.in_list("b", [V.Boolean(None), V.Int8(1)]), 6),
                           (P.in_list("d", [V.Int64(1)]), 7), (P.in_list("t", [V.TimestampNs(0), V.Int64(1)]), 7), (P.in_list("nope", [V.Int64(1)]), 101)):
            with pytest.raises(FM.FilterRefused) as e:
                IM.evaluate(pred, tab, leaf=leaf)
            assert e.value.code == code


def test_the_probe_of_a_table_built_by_hand():
    """eight slots, the keys 5, 9 and -1: the probe finds them and nothing else"""
    import struct
    slots, occ = [0] * 8, 0
    for key in (5, 9, 2 ** 64 - 1):
        s = IM.hash_i64(key) & 7
        while (occ >> s) & 1:
            s = (s + 1) & 7
        occ |= 1 << s
        slots[s] = key
    blob = struct.pack("<8I", IM.IN_KEY_I64, 8, 3, 0, 0, 0, 0, 0) + struct.pack("<Q", occ) + struct.pack("<8Q", *slots)
    t = IM.Table(blob)
    assert sorted(t.keys()) == [5, 9, 2 ** 64 - 1]
    assert t.probe(5)[0] and t.probe(9)[0] and t.probe(-1)[0] and not t.probe(0)[0] and not t.probe(6)[0]
    assert IM.float_key(-0.0) == IM.float_key(0.0) == 0 and IM.hash_bytes(b"") == IM.hash_bytes(b"") != IM.hash_bytes(b"\x00")
