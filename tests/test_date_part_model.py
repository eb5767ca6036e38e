"""tests/date_part_model.py judged by datetime.date and by numpy's datetime64, and its lowering of whole expressions onto the
existing models.  No GPU, no library."""
import datetime

import numpy as np
import pytest

import agg_expr_model as AEM
import date_part_model as M
from orc_rust_amd.aggregate import col, day, day_of_week, day_of_year, extract, month, quarter, year

EPOCH = datetime.date(1970, 1, 1).toordinal()
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SCHEMA = {"d": "date", "a": "int", "p": ("dec", 2)}


def fields(d):
    return d.year, (d.month - 1) // 3 + 1, d.month, d.day, d.isoweekday(), d.timetuple().tm_yday


def model_fields(days):
    return tuple(M.part_of(days, p) for p in range(6))


def test_every_13th_day_of_the_years_1_to_9999_is_datetime_dates():
    first, last = datetime.date(1, 1, 1).toordinal(), datetime.date(9999, 12, 31).toordinal()
    for o in list(range(first, last + 1, 13)) + [last]:
        assert model_fields(o - EPOCH) == fields(datetime.date.fromordinal(o)), o


def test_month_ends_and_the_century_years_february():
    for y in range(1, 10000, 7):
        for m in range(1, 13):
            first = datetime.date(y, m, 1)
            for d in (first, first - datetime.timedelta(days=1)) if (y, m) != (1, 1) else (first,):
                assert model_fields(d.toordinal() - EPOCH) == fields(d), d
    for y in range(100, 10000, 100):
        mar1 = datetime.date(y, 3, 1)
        for back in (0, 1, 2):  # 1 March, 28 or 29 February, the day before
            d = mar1 - datetime.timedelta(days=back)
            assert model_fields(d.toordinal() - EPOCH) == fields(d), d
        assert (M.part_of(mar1.toordinal() - EPOCH - 1, M.DAY) == 29) == (y % 400 == 0), y


def test_the_whole_int32_range_is_numpys():
    rng = np.random.default_rng(20261021)
    days = np.concatenate([np.arange(I32_MIN, I32_MAX, 40009, dtype=np.int64), rng.integers(I32_MIN, I32_MAX, 20000, dtype=np.int64),
                           np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], dtype=np.int64)])
    D = days.astype("datetime64[D]")
    Y, Mo = D.astype("datetime64[Y]"), D.astype("datetime64[M]")
    want_year = Y.astype(np.int64) + 1970
    want_month = Mo.astype(np.int64) - (want_year - 1970) * 12 + 1
    want_day = (D - Mo.astype("datetime64[D]")).astype(np.int64) + 1
    want_doy = (D - Y.astype("datetime64[D]")).astype(np.int64) + 1
    want_dow = (days + 3) % 7 + 1  # 1970-01-01 is a Thursday
    for k, d in enumerate(days.tolist()):
        y, q, m, dd, w, n = model_fields(d)
        assert (y, m, dd, n, w) == (want_year[k], want_month[k], want_day[k], want_doy[k], want_dow[k]), d
        assert q == (m - 1) // 3 + 1
    assert M.part_of(I32_MIN, M.YEAR) == -5877641 and M.part_of(I32_MAX, M.YEAR) == 5881580
    assert model_fields(0) == (1970, 1, 1, 1, 4, 1) and model_fields(-1) == (1969, 4, 12, 31, 3, 365) and model_fields(1)[3:5] == (2, 5)
    assert model_fields(-719528) == (0, 1, 1, 1, 6, 1)  # 0000-01-01: year 0 exists, and is a leap year
    assert M.part_of(-719528 + 59, M.DAY) == 29 and M.part_of(-719528 - 1, M.YEAR) == -1


def test_outside_int32_there_is_no_value():
    assert M.part_of(I32_MAX + 1, M.YEAR) is None and M.part_of(I32_MIN - 1, M.DAY) is None


def test_the_lowering_hands_plain_columns_to_the_models():
    e = year(col("d") + col("a")) * 100 + month("d")
    low, row, over = M.lower(e, {"d": 9131, "a": 31})
    assert not over and not M.holds_date_part(low) and row["__dp0"] == 1995 and row["__dp1"] == 1
    assert M.computed_value(e, SCHEMA, {"d": 9131, "a": 31}) == (199501, False)
    assert M.computed_value(e, SCHEMA, {"d": 9131, "a": None}) == (None, False)
    assert M.computed_value(e, SCHEMA, {"d": I32_MAX, "a": 1}) == (None, True)  # the operand leaves int32
    assert M.computed_value(year(col("a") * col("a") * col("a")), SCHEMA, {"a": 2 ** 62}) == (None, True)  # ... leaves 128 bits
    assert M.computed_value(e, SCHEMA, {"d": None, "a": 2 ** 62}) == (None, False)  # NULL comes first
    assert M.computed_type(e, SCHEMA) == ("int64", 0) and M.computed_type(year("d") * col("p"), SCHEMA) == ("decimal128", 2)
    assert M.computed_value(year("d") * col("p"), SCHEMA, {"d": 0, "p": 150}) == (1970 * 150, False)
    assert M.computed_value(year(year("d")), SCHEMA, {"d": 9131}) == (1975, False)  # day 1995 is in 1975


def test_the_lowering_for_aggregates_and_filter_leaves():
    assert M.agg_row(day_of_year("d"), SCHEMA, {"d": 59}) == 60 and M.agg_row(year(col("d") + 1), SCHEMA, {"d": I32_MAX}) == AEM.ROW_OVERFLOW
    assert M.agg_row(quarter("d"), SCHEMA, {"d": None}) is None
    assert M.filter_leaf(year("d"), "=", col("a"), {"d": 9131, "a": 1995}, SCHEMA) == (True, False)
    assert M.filter_leaf(month("d"), "<", quarter("d") * 3, {"d": 9131, "a": 0}, SCHEMA) == (True, False)
    assert M.filter_leaf(day("d"), "=", col("a"), {"d": None, "a": 1}, SCHEMA) == (None, False)
    assert M.filter_leaf(day_of_week(col("d") + col("a")), ">", 0, {"d": I32_MIN, "a": -1}, SCHEMA) == (None, True)
    assert M.filter_leaf(extract("day_of_week", "d"), "=", 4, {"d": 0, "a": 0}, SCHEMA) == (True, False)


@pytest.mark.parametrize("ymd,want", [((2000, 2, 29), (2000, 1, 2, 29, 2, 60)), ((1900, 2, 28), (1900, 1, 2, 28, 3, 59)), ((1900, 3, 1), (1900, 1, 3, 1, 4, 60)),
                                      ((1600, 2, 29), (1600, 1, 2, 29, 2, 60)), ((1600, 12, 31), (1600, 4, 12, 31, 7, 366))])
def test_the_leap_days_of_1600_1900_2000(ymd, want):
    assert model_fields(datetime.date(*ymd).toordinal() - EPOCH) == want
    assert (datetime.date(1900, 3, 1) - datetime.date(1900, 2, 28)).days == 1  # (1900 has no 29 February)
