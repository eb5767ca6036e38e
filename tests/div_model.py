"""The model of division in an expression (include/orcgpu.h: DIVISION; `/`, `//`, `%` and orc_rust_amd.aggregate.divide) in plain
Python ints and `fractions.Fraction`.

  a / b   exact: Q = round(A * 10^k / B), half away from zero, at the scale s the node names or min(38, max(6, sa + 4)), with
          k = s - sa + sb; the row overflows when B = 0, when A * 10^k leaves 128 bits or when Q does.  Doubles: one IEEE division.
  a // b  Python's floor division of integers; a % b Python's remainder (the divisor's sign).  b = 0 overflows the row.

Whole expressions go to the existing models unchanged: `lower` rewrites every division subtree of an expression into a synthetic
column that holds the model's value for the row at hand -- a Decimal column at the quotient's scale, an integer column for // and
%, a float column in a FLOAT expression -- and says whether one of them overflowed there.  tests/date_part_model.py (and through it
tests/computed_model.py, tests/agg_expr_model.py and tests/filter_model_expr.py) then sees no division.  A date part below a
division is the date-part model's.  TEST INFRASTRUCTURE: nothing here is used by the product."""
import fractions
import math
import struct

import agg_expr_model as AEM
import computed_model as CM
import date_part_model as DPM
from orc_rust_amd import aggregate as A

I128 = (-2 ** 127, 2 ** 127 - 1)
DIVISIONS = (A.EXPR_DIV, A.EXPR_FLOOR_DIV, A.EXPR_MOD)
SIGN = {A.EXPR_DIV: "/", A.EXPR_FLOOR_DIV: "//", A.EXPR_MOD: "%"}
DEFAULT_NAN = struct.unpack("<d", struct.pack("<Q", 0xfff8000000000000))[0]


def fits(v):
    return I128[0] <= v <= I128[1]


def result_scale(sa, scale=None):
    return min(38, max(6, sa + 4)) if scale is None else scale


def power_of(sa, sb, scale=None):
    """k of Q = round(A * 10^k / B), or Refused('unsupported') outside 0 .. 38"""
    k = result_scale(sa, scale) - sa + sb
    if not 0 <= k <= 38:
        raise AEM.Refused("unsupported", "scales %d, %d, %d" % (sa, sb, result_scale(sa, scale)))
    return k


def div_round(a, b, k=0):
    """round(a * 10^k / b), half away from zero; None: the row overflows"""
    if b == 0:
        return None
    n = a * 10 ** k
    if not fits(n):
        return None
    q = fractions.Fraction(n, b)
    m = abs(q)
    r = m.numerator // m.denominator
    if (m - r) * 2 >= 1:
        r += 1
    r = -r if q < 0 else r
    return r if fits(r) else None


def floor_div(a, b):
    if b == 0:
        return None
    q = a // b
    return q if fits(q) else None


def mod(a, b):
    return None if b == 0 else a % b


def float_div(a, b):
    """one IEEE double division: Python's, with the zero divisor Python raises on spelled out.  0 / 0 is the default NaN of the
    x86 host and of gfx950's division alike, the one with the sign bit set; a NaN dividend comes back quieted, as from any operation"""
    if b == 0.0:
        if math.isnan(a):
            return a + 0.0
        if a == 0.0:
            return DEFAULT_NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def holds_division(e):
    return e.op in DIVISIONS or any(holds_division(c) for c in e.children)


def is_float(exprs, schema):
    """whether the expressions (typed together) are of the FLOAT class"""
    leaves = [x for e in exprs for x in AEM.leaves(e)]
    cols = [x for x in leaves if x.op == A.EXPR_COLUMN]
    if any(schema[c.column] == "float" for c in cols):
        return True
    return not cols and any(x.op == A.EXPR_LITERAL and x.value_type == A.PV_FLOAT64 for x in leaves)


def lower(e, schema, row, prefix="__dv", floating=None):
    """-> (the expression with every division subtree replaced by a synthetic column, the schema with those columns, the row with
    their values, whether a division overflowed on this row).  The caller has seen to it that no column of e is NULL in the row."""
    schema, out = dict(schema), dict(row)
    floating = is_float([e], schema) if floating is None else floating
    state = {"over": False, "n": 0}

    def value_of(x):  # a division-free operand -> (unscaled, scale), or None when it overflows
        low, row2, over = DPM.lower(x, out, prefix + "p%d_" % state["n"])
        if over:
            return None
        s2 = dict(schema)
        for name in row2:
            s2.setdefault(name, "int")
        try:
            return AEM._exact(low, row2, CM.scales_of(s2))
        except AEM._Overflow:
            return None

    def walk(x):
        if not x.children:
            return x
        kids = [walk(c) for c in x.children]
        if x.op not in DIVISIONS:
            return A.Expr(x.op, kids, x.column, x.value_type, x.value, x.part, x.scale)
        name = "%s%d" % (prefix, state["n"])
        state["n"] += 1
        if floating:
            if x.op != A.EXPR_DIV:
                raise AEM.Refused("mismatched", "%s in a Float / Double expression" % SIGN[x.op])
            schema[name] = "float"
            out[name] = float_div(AEM._float(kids[0], out), AEM._float(kids[1], out))
            return A.col(name)
        # the scales do not depend on the row
        sa, sb = (AEM.scale_of(k, CM.scales_of(schema)) for k in (DPM.lower(k, {leaf.column: 0 for leaf in AEM.leaves(k) if leaf.op == A.EXPR_COLUMN})[0] for k in kids))
        if x.op == A.EXPR_DIV:
            k = power_of(sa, sb, x.scale)
            schema[name] = ("dec", result_scale(sa, x.scale))
        else:
            if sa or sb:
                raise AEM.Refused("mismatched", "%s on an operand of a non-zero scale" % SIGN[x.op])
            schema[name] = "int"
        a, b = value_of(kids[0]), value_of(kids[1])
        v = None
        if a is not None and b is not None:
            v = div_round(a[0], b[0], k) if x.op == A.EXPR_DIV else floor_div(a[0], b[0]) if x.op == A.EXPR_FLOOR_DIV else mod(a[0], b[0])
        state["over"] |= v is None
        out[name] = 0 if v is None else v
        return A.col(name)

    return walk(e), schema, out, state["over"]


def _null(e, row):
    return any(row[leaf.column] is None for leaf in AEM.leaves(e) if leaf.op == A.EXPR_COLUMN)


def _zero_row(e):
    return {leaf.column: 0 for leaf in AEM.leaves(e) if leaf.op == A.EXPR_COLUMN}


def computed_type(e, schema):
    """(CM.INT64 | CM.DEC128 | CM.FLOAT64, scale) of a computed column with divisions"""
    low, s2, _, _ = lower(e, schema, _zero_row(e))
    return DPM.computed_type(low, s2)


def computed_value(e, schema, row):
    """(value, overflowed) of a computed column on one row: None, False for NULL; None, True for an overflow"""
    if _null(e, row):
        return None, False
    low, s2, row2, over = lower(e, schema, row)
    if over:
        return None, True
    return DPM.computed_value(low, s2, row2)


def computed_column(e, schema, rows):
    vals, over = [], 0
    for row in rows:
        v, o = computed_value(e, schema, row)
        vals.append(v)
        over += 1 if o else 0
    return vals, over


def agg_row(e, schema, row):
    """what an expression aggregate sees of a row: None (NULL), AEM.ROW_OVERFLOW, the unscaled int, or the float"""
    if _null(e, row):
        return None
    low, s2, row2, over = lower(e, schema, row)
    if over:
        return AEM.ROW_OVERFLOW
    return DPM.agg_row(low, s2, row2)


def agg_scale(e, schema):
    return computed_type(e, schema)[1]


def filter_leaf(lhs, op, rhs, row, schema):
    """(True / False / None, overflowed) of lhs OP rhs on one row; the two sides are typed together"""
    lhs, rhs = A.Expr._wrap(lhs), A.Expr._wrap(rhs)
    if _null(lhs, row) or _null(rhs, row):
        return None, False
    floating = is_float([lhs, rhs], schema)
    l, s2, row2, over_l = lower(lhs, schema, row, "__dvl", floating)
    r, s3, row3, over_r = lower(rhs, s2, row2, "__dvr", floating)
    if over_l or over_r:
        return None, True
    return DPM.filter_leaf(l, op, r, row3, s3)
