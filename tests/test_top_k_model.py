"""The model of ORDER BY ... LIMIT k (tests/top_k_model.py) on hand cases whose expected order is spelled out here, rule by rule of
include/orcgpu.h ("Top-k").  No GPU."""
import decimal

import top_k_model as M

NAN, INF = float("nan"), float("inf")
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def order(values, descending=False, nulls_first=False, k=None):
    rows = [{"x": v} for v in values]
    return M.top_k_order(rows, [("x", descending, nulls_first)], len(rows) if k is None else k)


def test_nan_sorts_above_inf_and_every_nan_is_equal():
    #         0    1     2     3    4     5
    values = [NAN, INF, -INF, 1.5, -NAN, 0.0]
    assert order(values) == [2, 5, 3, 1, 0, 4]               # -inf < 0 < 1.5 < +inf < NaN = NaN (by row)
    assert order(values, descending=True) == [0, 4, 1, 3, 5, 2]


def test_negative_zero_equals_zero_and_rows_decide():
    values = [0.0, -0.0, -0.0, 0.0, -1.0]
    assert order(values) == [4, 0, 1, 2, 3]
    assert order(values, descending=True) == [0, 1, 2, 3, 4]  # the zeros are tied: input order, also descending


def test_nulls_first_under_descending_and_nulls_last_by_default():
    values = [3, None, 1, None, 2]
    assert order(values) == [2, 4, 0, 1, 3]
    assert order(values, descending=True) == [0, 4, 2, 1, 3]                       # `descending` does not move the NULLs
    assert order(values, descending=True, nulls_first=True) == [1, 3, 0, 4, 2]
    assert order(values, nulls_first=True) == [1, 3, 2, 4, 0]


def test_int64_extremes():
    values = [0, INT64_MAX, INT64_MIN, -1, 1]
    assert order(values) == [2, 3, 0, 4, 1]
    assert order(values, descending=True) == [1, 4, 0, 3, 2]


def test_a_negative_decimal38_against_a_positive_one():
    big = decimal.Decimal(10 ** 37)
    values = [big, -big, decimal.Decimal(0), decimal.Decimal(-1), None]
    assert order(values) == [1, 3, 2, 0, 4]
    assert order(values, descending=True, nulls_first=True) == [4, 0, 2, 3, 1]


def test_booleans():
    assert order([True, False, None, True, False]) == [1, 4, 0, 3, 2]


def test_four_keys_where_only_the_last_differs():
    rows = [{"a": 1, "b": 2.5, "c": True, "d": d} for d in (5, 3, None, 4, 3)]
    keys = [("a", False, False), ("b", True, False), ("c", False, True), ("d", False, False)]
    assert M.top_k_order(rows, keys, 5) == [1, 4, 3, 0, 2]
    keys[3] = ("d", True, True)
    assert M.top_k_order(rows, keys, 3) == [2, 0, 3]


def test_k_cuts_after_the_stable_sort_and_kept_rows_only():
    values = [2, 1, 2, 1, 2, 1]
    assert order(values, k=4) == [1, 3, 5, 0]
    rows = [{"x": v} for v in values]
    assert M.top_k_order(rows, [("x", False, False)], 2, kept=[True, False, True, False, True, True]) == [5, 0]
    assert M.top_k_order(rows, [("x", False, False)], 9, kept=[False] * 6) == []
