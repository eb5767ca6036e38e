"""The model of the row filter's Decimal and Timestamp leaves (include/orcgpu.h, orcgpu_result_filter), around filter_model: a
Decimal column against a Decimal128 literal as two exact fractions, a Timestamp column against a TimestampNs literal as two
integers of nanoseconds.  Python's own arithmetic only: no rescaling to a common scale, no int128, no floor -- nothing the
product does on the way.  TEST INFRASTRUCTURE: nothing here is used by the product."""
from fractions import Fraction

import numpy as np
import pyarrow as pa

import filter_model as FM
from orc_rust_amd import predicate as PR

NS_PER_UNIT = {"s": 10 ** 9, "ms": 10 ** 6, "us": 10 ** 3, "ns": 1}


def _typed_leaf(pred, col):
    """(t, f) of a comparison on a Decimal or Timestamp column."""
    n = len(col)
    kind, lit = pred.value.kind, pred.value.value
    t, f = np.zeros(n, bool), np.zeros(n, bool)
    if pa.types.is_decimal(col.type):
        if kind != PR.PV_DECIMAL128:
            raise FM.FilterRefused(7, "Decimal column %r against a literal of kind %d" % (pred.column, kind))
        if lit is None:
            return t, f
        lit = Fraction(lit[0], 10 ** lit[1])
        values = [None if v is None else Fraction(v) for v in col.to_pylist()]
    else:
        if kind != PR.PV_TIMESTAMP_NS:
            raise FM.FilterRefused(7, "Timestamp column %r against a literal of kind %d" % (pred.column, kind))
        if lit is None:
            return t, f
        per = NS_PER_UNIT[col.type.unit]
        values = [None if v is None else v * per for v in col.cast(pa.int64()).to_pylist()]
    for k, v in enumerate(values):
        if v is not None:
            r = bool(FM._compare(pred.op, v, lit))
            t[k], f[k] = r, not r
    return t, f


def evaluate(pred, table):
    """-> (t, f) over the table's rows; everything but the two new leaves is filter_model's."""
    n = table.num_rows
    if pred.op == PR.AND:
        acc = (np.ones(n, bool), np.zeros(n, bool))
        for c in pred.children:
            acc = FM.and3(acc, evaluate(c, table))
        return acc
    if pred.op == PR.OR:
        acc = (np.zeros(n, bool), np.ones(n, bool))
        for c in pred.children:
            acc = FM.or3(acc, evaluate(c, table))
        return acc
    if pred.op == PR.NOT:
        return FM.not3(evaluate(pred.children[0], table))
    if pred.op <= PR.GE and pred.column in table.column_names:
        col = table.column(pred.column)
        if pa.types.is_decimal(col.type) or pa.types.is_timestamp(col.type):
            return _typed_leaf(pred, col)
    return FM.evaluate(pred, table)


def keep_mask(pred, table):
    return evaluate(pred, table)[0]


def filter_table(table, pred):
    return table.filter(pa.array(keep_mask(pred, table)))


def expected_batches(table, pred, stripe_rows, batch_size, selection_batches=None):
    """filter_model.expected_batches under this model."""
    out, base = [], 0
    for k, n in enumerate(stripe_rows):
        stripe = table.slice(base, n)
        if selection_batches is not None and selection_batches[k] is not None:
            parts = [stripe.slice(s, m) for s, m in selection_batches[k]]
            stripe = pa.concat_tables(parts) if parts else stripe.slice(0, 0)
        kept = filter_table(stripe, pred)
        out += FM.rebatch(kept, [kept.num_rows], batch_size)
        base += n
    return out
