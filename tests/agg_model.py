"""The model of the aggregates over the kept rows (include/orcgpu.h, orcgpu_result_aggregate), in plain Python: Python ints and
`decimal` for everything exact, `math.fsum` for the float sums, the NaN rule of MIN / MAX by hand.  The kept-row mask is the
row filter's model's (tests/filter_model.py, filter_model_typed.py, in_model.py) and-ed with the row selection's
(tests/selection_model.py).  TEST INFRASTRUCTURE: nothing here is used by the product."""
import decimal
import math

import numpy as np
import pyarrow as pa

import in_model as IM
import selection_model as SM
from orc_rust_amd import aggregate as A

OVERFLOW = "overflow"   # what a result with the overflow flag set is to the model
NS_PER = {"s": 10 ** 9, "ms": 10 ** 6, "us": 10 ** 3, "ns": 1}
EXACT = decimal.Context(prec=80)
I64 = (-2 ** 63, 2 ** 63 - 1)


def kept_mask(table, pred=None, selectors=None, batch_size=1024):
    """bool per row: selected by the row selection (if any) and TRUE under the predicate (if any)"""
    n = table.num_rows
    keep = np.ones(n, bool)
    if selectors is not None:
        keep[:] = False
        ranges = SM.file_batches(selectors, [n], batch_size)[0]
        for start, length in [(0, n)] if ranges is None else ranges:   # (None: a selection of no rows does not apply)
            keep[start:start + length] = True
    if pred is not None:
        keep &= IM.evaluate(pred, table)[0]
    return keep


_VALUES = {}


def column_values(table, name, ts_unit="ns"):
    """column_values_of(table.column(name)), remembered per table: a test asks for the same column under many specs and masks"""
    key = (id(table), name, ts_unit)
    if key not in _VALUES or _VALUES[key][0] is not table:
        if len(_VALUES) > 256:
            _VALUES.clear()
        _VALUES[key] = (table, column_values_of(table.column(name), ts_unit))
    return _VALUES[key][1]


def column_values_of(col, ts_unit="ns"):
    """(values with None for nulls, family, scale): family 'int' (Byte .. Long) | 'date' | 'bool' | 'float' | 'decimal' (unscaled
    ints) | 'timestamp' (ints in ts_unit) | 'other'"""
    t = col.type
    if pa.types.is_integer(t):
        return col.to_pylist(), "int", 0
    if pa.types.is_date32(t):
        return col.cast(pa.int32()).to_pylist(), "date", 0
    if pa.types.is_boolean(t):
        return [None if v is None else int(v) for v in col.to_pylist()], "bool", 0
    if pa.types.is_floating(t):
        return col.to_pylist(), "float", 0
    if pa.types.is_decimal(t):
        return [None if v is None else int(v.scaleb(t.scale, EXACT)) for v in col.to_pylist()], "decimal", t.scale
    if pa.types.is_timestamp(t):
        per = NS_PER[t.unit]
        return [None if v is None else v * per // NS_PER[ts_unit] for v in col.cast(pa.int64()).to_pylist()], "timestamp", 0
    return [None if not ok else 0 for ok in col.is_valid().to_pylist()], "other", 0


def float_sum(xs):
    """IEEE: a NaN, or infinities of both signs, give NaN; one sign of infinity gives it; else the exactly rounded sum"""
    if any(x != x for x in xs) or (math.inf in xs and -math.inf in xs):
        return math.nan
    for inf in (math.inf, -math.inf):
        if inf in xs:
            return inf
    return math.fsum(xs)


def float_minmax(xs, is_max):
    """NaN values are skipped unless every value is NaN"""
    real = [x for x in xs if x == x]
    if not real:
        return math.nan
    return max(real) if is_max else min(real)


def _decimal(unscaled, scale):
    return OVERFLOW if abs(unscaled) >= 10 ** 38 else decimal.Decimal(unscaled).scaleb(-scale, EXACT)


def _int128(v):
    return v if -2 ** 127 <= v < 2 ** 127 else OVERFLOW


def float_terms(table, spec, keep):
    """the doubles a float SUM / SUM_PRODUCT adds up: what float_bound is taken of"""
    vals = column_values(table, spec.column)[0]
    if spec.op == A.SUM_PRODUCT:
        vals2 = column_values(table, spec.column2)[0]
        return [a * b for a, b, k in zip(vals, vals2, keep) if k and a is not None and b is not None]
    return [v for v, k in zip(vals, keep) if k and v is not None]


def aggregate_one(table, spec, keep, ts_unit="ns"):
    if spec.op == A.COUNT_ROWS:
        return int(keep.sum())
    vals, family, scale = column_values(table, spec.column, ts_unit)
    rows = [v for v, k in zip(vals, keep) if k and v is not None]
    if spec.op == A.COUNT:
        return len(rows)
    if spec.op == A.SUM_PRODUCT:
        vals2, family2, scale2 = column_values(table, spec.column2, ts_unit)
        assert family == family2 and family in ("int", "float", "decimal"), (family, family2)
        pairs = [(a, b) for a, b, k in zip(vals, vals2, keep) if k and a is not None and b is not None]
        if not pairs:
            return None
        if family == "float":
            return float_sum([a * b for a, b in pairs])
        if family == "decimal":
            if any(not (I64[0] <= a <= I64[1] and I64[0] <= b <= I64[1]) for a, b in pairs):
                return OVERFLOW
            return _decimal(sum(a * b for a, b in pairs), scale + scale2)
        return _int128(sum(a * b for a, b in pairs))
    if not rows:
        return None
    if spec.op == A.SUM:
        assert family in ("int", "float", "decimal"), family
        return float_sum(rows) if family == "float" else _decimal(sum(rows), scale) if family == "decimal" else _int128(sum(rows))
    assert family != "other", family
    is_max = spec.op == A.MAX
    if family == "float":
        return float_minmax(rows, is_max)
    v = max(rows) if is_max else min(rows)
    return decimal.Decimal(v).scaleb(-scale, EXACT) if family == "decimal" else v


def aggregate(table, specs, pred=None, selectors=None, batch_size=1024, ts_unit="ns", keep=None):
    """The list orcgpu_result_aggregate / ArrowReaderBuilder.aggregate give for `table`: ints, decimal.Decimal, floats, None for
    NULL, OVERFLOW where the call raises OverflowError."""
    if keep is None:
        keep = kept_mask(table, pred, selectors, batch_size)
    return [aggregate_one(table, s, keep, ts_unit) for s in specs]


def float_bound(xs):
    """|got - fsum(x)| <= 2 n 2^-53 fsum(|x|): the textbook bound for a sum of n doubles in any order (each of the n - 1 additions
    rounds once; (1 + u)^(n-1) - 1 <= 2 n u while n u < 0.1)"""
    return 2 * len(xs) * 2.0 ** -53 * math.fsum(abs(x) for x in xs)


def same(got, want):
    """equal as results: NaN equals NaN, -0.0 equals 0.0"""
    if isinstance(want, float) and isinstance(got, float):
        return (got != got and want != want) or got == want
    return type(got) is type(want) and got == want if not isinstance(want, int) else isinstance(got, int) and got == want
