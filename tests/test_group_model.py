"""tests/group_model.py against hand-written tables: first-appearance order, NULL keys, 0 / NULL / '' as three keys, Char padding,
no kept row, the data-dependent refusals."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

import agg_model as AM
import group_model as GM
from orc_rust_amd.aggregate import Agg

D = decimal.Decimal


def test_order_is_first_appearance_and_values_are_per_group():
    t = pa.table({"k": pa.array(["b", "a", "b", None, "a", None, "c"]), "v": pa.array([1, 2, 3, 4, None, 6, 7], pa.int64())})
    got = GM.aggregate_groups(t, [Agg.count_rows(), Agg.sum("v"), Agg.count("v"), Agg.min("v")], ["k"])
    assert got == [(("b",), [2, 4, 2, 1]), (("a",), [2, 2, 1, 2]), ((None,), [2, 10, 2, 4]), (("c",), [1, 7, 1, 7])]
    keep = np.array([0, 0, 1, 0, 1, 0, 1], bool)              # the order is that of the KEPT rows
    got = GM.aggregate_groups(t, [Agg.count_rows(), Agg.sum("v")], ["k"], keep=keep)
    assert got == [(("b",), [1, 3]), (("a",), [1, None]), (("c",), [1, 7])]


def test_zero_null_and_the_empty_string_are_three_keys():
    t = pa.table({"i": pa.array([0, None, 0, None], pa.int64()), "s": pa.array(["", "", None, None]), "b": pa.array([False, None, False, True])})
    assert [k for k, _ in GM.aggregate_groups(t, [Agg.count_rows()], ["i", "s"])] == [(0, ""), (None, ""), (0, None), (None, None)]
    assert [k for k, _ in GM.aggregate_groups(t, [Agg.count_rows()], ["b"])] == [(False,), (None,), (True,)]
    assert GM.key_id(False) != GM.key_id(0) != GM.key_id("")


def test_char_padding_is_part_of_the_key():
    t = pa.table({"c": pa.array(["a  ", "a", "a  ", "a "]), "v": pa.array([1, 2, 3, 4], pa.int64())})
    assert GM.aggregate_groups(t, [Agg.sum("v")], ["c"]) == [(("a  ",), [4]), (("a",), [2]), (("a ",), [4])]


def test_no_kept_row_is_no_group():
    t = pa.table({"k": pa.array([1, 2], pa.int64())})
    assert GM.aggregate_groups(t, [Agg.count_rows()], ["k"], keep=np.zeros(2, bool)) == []
    assert GM.aggregate_groups(t.slice(0, 0), [Agg.count_rows()], ["k"]) == []


def test_decimal_date_and_timestamp_keys():
    t = pa.table({"d": pa.array([D("1.50"), D("-1.50"), D("1.50"), None], pa.decimal128(10, 2)), "day": pa.array([3, 3, -4, 3], pa.date32()),
                  "ts": pa.array([10 ** 9, 10 ** 9, 5, None], pa.timestamp("ns"))})
    assert [k for k, _ in GM.aggregate_groups(t, [Agg.count_rows()], ["d"])] == [(D("1.50"),), (D("-1.50"),), (None,)]
    assert [k for k, _ in GM.aggregate_groups(t, [Agg.count_rows()], ["day", "ts"])] == [(3, 10 ** 9), (-4, 5), (3, None)]
    assert [k for k, _ in GM.aggregate_groups(t, [Agg.count_rows()], ["ts"], ts_unit="us")] == [(10 ** 6,), (0,), (None,)]
    with pytest.raises(TypeError):
        GM.aggregate_groups(pa.table({"f": pa.array([1.0])}), [Agg.count_rows()], ["f"])


def test_the_overflow_of_one_group_stays_in_it():
    big = D(10 ** 38 - 1)
    t = pa.table({"k": pa.array([1, 1, 2], pa.int64()), "d": pa.array([big, D(1), D(5)], pa.decimal128(38, 0))})
    assert GM.aggregate_groups(t, [Agg.sum("d")], ["k"]) == [((1,), [AM.OVERFLOW]), ((2,), [D(5)])]


def test_limits():
    t = pa.table({"k": pa.array(np.arange(257), pa.int64()), "s": pa.array(["x" * 65] + ["y" * 64] * 256)})
    assert GM.aggregate_groups(t, [Agg.count_rows()], ["k"]) == GM.TOO_MANY
    assert len(GM.aggregate_groups(t.slice(0, 256), [Agg.count_rows()], ["k"])) == 256
    assert GM.aggregate_groups(t, [Agg.count_rows()], ["s"]) == GM.KEY_TOO_LONG
    keep = np.ones(257, bool)
    keep[0] = False                                         # the long value only among the rows that are dropped
    assert GM.aggregate_groups(t, [Agg.count_rows()], ["s"], keep=keep) == [(("y" * 64,), [256])]
    assert GM.merge_stripes([[((1,), []), ((2,), [])], [((2,), []), ((0,), [])], [((None,), []), ((1,), [])]]) == [(1,), (2,), (0,), (None,)]
