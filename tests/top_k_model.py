"""A plain Python model of ORDER BY ... LIMIT k as include/orcgpu.h ("Top-k") fixes it: a key function that maps a row to a tuple
under the rules there, and `sorted` -- which is stable -- over the kept rows in input order.  TEST INFRASTRUCTURE: the GPU tests
judge the library against this, row for row.

A key is (column, descending, nulls_first); a row is a dict column -> Python value (None: NULL).  Values: int (a Date as its days,
a Timestamp as its int64 unit), bool, decimal.Decimal (or the unscaled int: one column has one scale, so either orders alike), float.
"""
import decimal
import math


def value_rank(v, descending):
    """A non-null value -> something Python orders as the header says: integers, Booleans and Decimals as they are; floats in
    the total order -inf < finite < +inf < NaN with every NaN equal and -0.0 = 0.0.  `descending` reverses it."""
    if isinstance(v, float):
        r = (1, 0.0) if math.isnan(v) else (0, v + 0.0 if v != 0 else 0.0)
        return (-r[0], -r[1]) if descending else r
    if isinstance(v, bool):
        v = int(v)
    if isinstance(v, decimal.Decimal):
        return v.copy_negate() if descending else v      # (unary minus would round to the context's 28 digits)
    return -v if descending else v


def row_key(row, keys):
    out = []
    for column, descending, nulls_first in keys:
        v = row[column]
        if v is None:
            out.append((0 if nulls_first else 2, 0))
        else:
            out.append((1, value_rank(v, descending)))
    return tuple(out)


def top_k_order(rows, keys, k, kept=None):
    """The indexes into `rows` (dicts, in input order) of the answer, in order.  kept: a list of bools, None: every row."""
    idx = [i for i in range(len(rows)) if kept is None or kept[i]]
    return sorted(idx, key=lambda i: row_key(rows[i], keys))[:k]


def key_values(column):
    """A pyarrow column as the values the model orders: a Timestamp as its int64 unit, a Date as its days"""
    import pyarrow as pa
    if pa.types.is_timestamp(column.type):
        column = column.cast(pa.int64())
    if pa.types.is_date32(column.type):
        column = column.cast(pa.int32())
    return column.to_pylist()


def top_k_table(table, keys, k, kept=None):
    """The same over a pyarrow.Table: the answer as a Table, every column."""
    import pyarrow as pa
    cols = {}
    for column, _, _ in keys:
        cols[column] = key_values(table.column(column))
    n = table.num_rows
    rows = [{c: cols[c][i] for c in cols} for i in range(n)]
    order = top_k_order(rows, keys, k, kept)
    return table.take(pa.array(order, type=pa.int64())), order
