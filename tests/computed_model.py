"""The model of computed columns (include/orcgpu.h: "Computed columns") in plain Python, on tests/agg_expr_model.py: the output
type and scale of an expression, a row's value, the NULL rule, the three overflow cases and their count.  Integers and Decimals
are Python ints (a Decimal's unscaled value); doubles are Python floats, rounded after every operation, compared by their bits.
TEST INFRASTRUCTURE: nothing here is used by the product."""
import struct

import agg_expr_model as AEM
from orc_rust_amd import aggregate as A

I64 = (-2 ** 63, 2 ** 63 - 1)
DEC_LIMIT = 10 ** 38
INT64, DEC128, FLOAT64 = "int64", "decimal128", "float64"


def families_of(schema):
    """schema: name -> 'int' | 'date' | 'float' | ('dec', scale) | anything else -> what agg_expr_model.classify reads (a Date
    takes part as int64 days)"""
    out = {}
    for name, t in schema.items():
        out[name] = "decimal" if isinstance(t, tuple) else "int" if t in ("int", "date") else t
    return out


def scales_of(schema):
    return {name: t[1] for name, t in schema.items() if isinstance(t, tuple)}


def output_type(e, schema):
    """(INT64 | DEC128 | FLOAT64, scale) of expression e over the schema, or agg_expr_model.Refused"""
    cls = AEM.classify(e, families_of(schema))
    if cls == AEM.FLOAT:
        return FLOAT64, 0
    if cls == AEM.DEC:
        return DEC128, AEM.scale_of(e, scales_of(schema))
    return INT64, 0


def eval_value(e, schema, row):
    """(value, overflowed): value None for NULL -- an operand is NULL (overflowed False), or the exact result does not fit
    (overflowed True: an operation left 128 bits, an Int64 result left int64, a Decimal reached 10^38)"""
    kind, _ = output_type(e, schema)
    cls = AEM.FLOAT if kind == FLOAT64 else AEM.DEC if kind == DEC128 else AEM.INT
    v = AEM.eval_row(e, cls, row, scales_of(schema))
    if v is None:
        return None, False
    if kind == FLOAT64:
        return v, False
    if v == AEM.ROW_OVERFLOW:
        return None, True
    if kind == INT64 and not I64[0] <= v <= I64[1]:
        return None, True
    if kind == DEC128 and abs(v) >= DEC_LIMIT:
        return None, True
    return v, False


def eval_column(e, schema, rows):
    """rows: a list of {column: value or None} -> (the column's values, the overflow count)"""
    out, over = [], 0
    for row in rows:
        v, o = eval_value(e, schema, row)
        out.append(v)
        over += 1 if o else 0
    return out, over


def bits(x):
    """a double's bit pattern; None stays None"""
    return None if x is None else struct.unpack("<Q", struct.pack("<d", x))[0]


def check_names(names, file_roots):
    """the refusals of the names: 'empty' | 'twice' | 'root' | None"""
    seen = set()
    for n in names:
        if not n:
            return "empty"
        if n in seen:
            return "twice"
        if n in file_roots:
            return "root"
        seen.add(n)
    return None


__all__ = ["A"]
