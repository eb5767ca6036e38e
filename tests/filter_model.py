"""A plain-Python / numpy model of the row filter (include/orcgpu.h, orcgpu_result_filter): a three-valued evaluator of
orc_rust_amd.predicate.Predicate over a pyarrow.Table, the batches a filtered reader hands out, and the inputs the tests of the
filter share (a table with every comparable type, seeded random predicates).  TEST INFRASTRUCTURE: nothing here is used by the
product.

A truth value is a pair of numpy bool arrays (t, f): TRUE where t, FALSE where f, UNKNOWN where neither."""
import datetime
import decimal

import numpy as np
import pyarrow as pa

from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

INT_KINDS = (PR.PV_INT8, PR.PV_INT16, PR.PV_INT32, PR.PV_INT64)
FLOAT_KINDS = (PR.PV_FLOAT32, PR.PV_FLOAT64)


class FilterRefused(Exception):
    """What the library answers with a status instead of batches: .code is that status."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def and3(a, b):
    return a[0] & b[0], a[1] | b[1]


def or3(a, b):
    return a[0] | b[0], a[1] & b[1]


def not3(a):
    return a[1], a[0]


def _compare(op, v, lit):
    """Python's own comparisons: IEEE for floats (a NaN makes all but != false), bytes by unsigned byte with the shorter one
    the smaller on a common prefix, False < True."""
    if op == PR.EQ:
        return v == lit
    if op == PR.NE:
        return v != lit
    if op == PR.LT:
        return v < lit
    if op == PR.LE:
        return v <= lit
    if op == PR.GT:
        return v > lit
    return v >= lit


def _column_values(col):
    """(python values with None for nulls, family) of a ChunkedArray; family: 'int' | 'float' | 'bool' | 'bytes' | 'date' | 'other'"""
    t = col.type
    if pa.types.is_integer(t):
        return col.to_pylist(), "int"
    if pa.types.is_floating(t):
        return col.to_pylist(), "float"  # (a float32 value as the double it is exactly)
    if pa.types.is_boolean(t):
        return col.to_pylist(), "bool"
    if pa.types.is_date32(t):
        return col.cast(pa.int32()).to_pylist(), "date"
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return [None if v is None else v.encode() for v in col.to_pylist()], "bytes"
    if pa.types.is_binary(t) or pa.types.is_large_binary(t):
        return col.to_pylist(), "bytes"
    if pa.types.is_timestamp(t) or pa.types.is_decimal(t):
        return [None if not ok else 0 for ok in col.is_valid().to_pylist()], "other"
    raise FilterRefused(7, "nested column")


def evaluate(pred, table):
    """-> (t, f) over the table's rows."""
    n = table.num_rows
    if pred.op == PR.AND:
        acc = (np.ones(n, bool), np.zeros(n, bool))
        for c in pred.children:
            acc = and3(acc, evaluate(c, table))
        return acc
    if pred.op == PR.OR:
        acc = (np.zeros(n, bool), np.ones(n, bool))
        for c in pred.children:
            acc = or3(acc, evaluate(c, table))
        return acc
    if pred.op == PR.NOT:
        return not3(evaluate(pred.children[0], table))
    if pred.column not in table.column_names:
        raise FilterRefused(101, "column %r is not there" % pred.column)
    values, family = _column_values(table.column(pred.column))
    valid = np.array([v is not None for v in values], bool).reshape(n)
    if pred.op == PR.IS_NULL:
        return ~valid, valid.copy()
    if pred.op == PR.IS_NOT_NULL:
        return valid.copy(), ~valid
    kind, lit = pred.value.kind, pred.value.value
    if family == "other":
        raise FilterRefused(7, "comparison on Timestamp / Decimal column %r" % pred.column)
    ok = {"int": kind in INT_KINDS, "date": kind in (PR.PV_INT32, PR.PV_INT64), "float": kind in FLOAT_KINDS, "bool": kind == PR.PV_BOOLEAN,
          "bytes": kind == PR.PV_UTF8}[family]
    if not ok:
        raise FilterRefused(6, "column %r against a literal of kind %d" % (pred.column, kind))
    t, f = np.zeros(n, bool), np.zeros(n, bool)
    if lit is None:
        return t, f  # a comparison with NULL is UNKNOWN on every row
    if kind == PR.PV_FLOAT32:
        lit = float(np.float32(lit))
    elif kind in FLOAT_KINDS:
        lit = float(lit)
    elif kind == PR.PV_UTF8:
        lit = lit.encode() if isinstance(lit, str) else bytes(lit)
    elif kind == PR.PV_BOOLEAN:
        lit = bool(lit)
    for k, v in enumerate(values):
        if v is not None:
            r = bool(_compare(pred.op, v, lit))
            t[k], f[k] = r, not r
    return t, f


def keep_mask(pred, table):
    return evaluate(pred, table)[0]


def filter_table(table, pred):
    return table.filter(pa.array(keep_mask(pred, table)))


def depth(pred):
    return 1 + max([depth(c) for c in pred.children] or [0])


def rebatch(table, stripe_rows, batch_size):
    """The table's rows as the reader's batches: every stripe's rows in batches of batch_size, its last one shorter; a stripe
    without rows yields none.  stripe_rows: rows of `table` that belong to each stripe."""
    out, base = [], 0
    for n in stripe_rows:
        for s in range(0, n, batch_size):
            out.append(table.slice(base + s, min(batch_size, n - s)))
        base += n
    assert base == table.num_rows
    return out


def expected_batches(table, pred, stripe_rows, batch_size, selection_batches=None):
    """What a reader with the row filter `pred` hands out: per stripe the kept rows of its (selected) rows, rebatched.
    selection_batches: per stripe [(start, len)] or None (selection_model.file_batches)."""
    out, base = [], 0
    for k, n in enumerate(stripe_rows):
        stripe = table.slice(base, n)
        if selection_batches is not None and selection_batches[k] is not None:
            parts = [stripe.slice(s, m) for s, m in selection_batches[k]]
            stripe = pa.concat_tables(parts) if parts else stripe.slice(0, 0)
        kept = filter_table(stripe, pred)
        out += rebatch(kept, [kept.num_rows], batch_size)
        base += n
    return out


# ---- shared inputs ------------------------------------------------------------------------------------------------------

LITERAL_STRING = "mango"


def make_table(n, seed=7):
    """Every comparable type with about 30 % nulls, an all-null column, columns without nulls (id, plain), special floats,
    strings around LITERAL_STRING (prefixes, extensions, empty, bytes >= 0x80, a few of 300+ bytes), and one Timestamp and
    one Decimal column for the null tests and the refusals."""
    rng = np.random.default_rng(seed)

    def nulls(values, frac=0.3):
        mask = rng.random(n) < frac
        return [None if m else v for v, m in zip(values, mask)]

    specials = [float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 1.5, -1.5]
    f64 = [specials[k] if k < len(specials) else float(x) for k, x in zip(rng.integers(0, 24, n), rng.normal(0, 3, n).round(1))]
    f32 = [specials[k] if k < len(specials) else float(np.float32(x)) for k, x in zip(rng.integers(0, 24, n), rng.normal(0, 3, n).round(1))]
    words = ["", "m", "man", "mang", "mango", "mangos", "mango\x00", "mangp", "manga", "apple", "zebra", "éclair", "mañana", "\U0001f96d",
             "x" * 300, "mango" + "y" * 330, "q" * 33, "r" * 32]
    s = [words[k] for k in rng.integers(0, len(words), n)]
    blobs = [b"", b"\x7f", b"\x80", b"\x7f\xff", b"\xff", b"mango", b"mang", b"\x00", b"\x80" * 301, b"ab"]
    bn = [blobs[k] for k in rng.integers(0, len(blobs), n)]
    day0 = datetime.date(1970, 1, 1)
    cols = {
        "id": pa.array(np.arange(n, dtype=np.int64)),
        "i8": pa.array(nulls(rng.integers(-128, 128, n).tolist()), pa.int8()),
        "i16": pa.array(nulls(rng.integers(-300, 300, n).tolist()), pa.int16()),
        "i32": pa.array(nulls(rng.integers(-5, 6, n).tolist()), pa.int32()),
        "i64": pa.array(nulls((rng.integers(-3, 4, n) * (1 << 40)).tolist()), pa.int64()),
        "f32": pa.array(nulls(f32), pa.float32()),
        "f64": pa.array(nulls(f64), pa.float64()),
        "b": pa.array(nulls((rng.random(n) < 0.5).tolist()), pa.bool_()),
        "d": pa.array(nulls([day0 + datetime.timedelta(days=int(x)) for x in rng.integers(-400, 400, n)]), pa.date32()),
        "s": pa.array(nulls(s), pa.string()),
        "bin": pa.array(nulls(bn), pa.binary()),
        "ts": pa.array(nulls([datetime.datetime(2020, 1, 1) + datetime.timedelta(seconds=int(x)) for x in rng.integers(0, 10 ** 7, n)]), pa.timestamp("ns")),
        "dec": pa.array(nulls([decimal.Decimal(int(x)) / 100 for x in rng.integers(-10 ** 6, 10 ** 6, n)]), pa.decimal128(10, 2)),
        "allnull": pa.array([None] * n, pa.int32()),
        "plain": pa.array(rng.integers(0, 100, n).astype(np.int32)),
    }
    return pa.table(cols)


COMPARABLE = ("id", "i8", "i16", "i32", "i64", "f32", "f64", "b", "d", "s", "bin", "allnull", "plain")
ALL_COLUMNS = COMPARABLE + ("ts", "dec")


def literal_for(table, name, value):
    """A PredicateValue of the kind the column takes, holding `value` (None: the NULL literal)."""
    t = table.schema.field(name).type
    if pa.types.is_integer(t):
        return {8: V.Int8, 16: V.Int16, 32: V.Int32, 64: V.Int64}[t.bit_width](value)
    if pa.types.is_float32(t):
        return V.Float32(value)
    if pa.types.is_floating(t):
        return V.Float64(value)
    if pa.types.is_boolean(t):
        return V.Boolean(value)
    if pa.types.is_date32(t):
        return V.Int32(None if value is None else (value - datetime.date(1970, 1, 1)).days if isinstance(value, datetime.date) else value)
    return V.Utf8(value)


def random_predicates(table, n, seed=11, max_depth=3):
    """n seeded predicates of depth <= max_depth over the table's comparable columns; the literals are the columns' own values,
    and now and then the NULL literal."""
    rng = np.random.default_rng(seed)
    pools = {c: [v for v in table.column(c).to_pylist() if v is not None] for c in COMPARABLE}

    def leaf():
        c = ALL_COLUMNS[rng.integers(0, len(ALL_COLUMNS))]
        roll = rng.random()
        if c in ("ts", "dec") or roll < 0.12:
            return P.is_null(c) if rng.random() < 0.5 else P.is_not_null(c)
        pool = pools[c]
        value = None if (roll < 0.2 or not pool) else pool[rng.integers(0, len(pool))]
        return P.comparison(c, int(rng.integers(0, 6)), literal_for(table, c, value))

    def node(d):
        if d <= 1 or rng.random() < 0.3:
            return leaf()
        roll = rng.random()
        if roll < 0.2:
            return P.not_(node(d - 1))
        kids = [node(d - 1) for _ in range(int(rng.integers(0, 4)))]
        return P.and_(kids) if roll < 0.6 else P.or_(kids)

    return [node(max_depth) for _ in range(n)]
