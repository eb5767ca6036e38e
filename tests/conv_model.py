"""The model of the conversions in an expression (include/orcgpu.h: CONVERSIONS; orc_rust_amd.aggregate.cast / round_ / floor /
ceil / trunc): a tree evaluator with the class decided PER NODE, over the existing models (tests/cond_model.py for the states and
Kleene's logic, tests/div_model.py, tests/date_part_model.py), written from the semantics, not from the C text.  Python ints,
`fractions.Fraction` and `float` (numpy float64 for the one-operation IEEE arithmetic).

A node's type is (class, scale): class 'int' | 'dec' | 'float' | 'cond'; its state on a row is None (NULL), OVER, (unscaled, scale)
for the exact classes, a float for 'float', True / False / None for a condition.  TEST INFRASTRUCTURE: nothing here is used by
the product."""
import math
from fractions import Fraction

import numpy as np

import agg_expr_model as AEM
import cond_model as CDM
import computed_model as CM
import date_part_model as DPM
import div_model as DM
from orc_rust_amd import aggregate as A
from orc_rust_amd import predicate as P

OVER = CDM.OVER
HALF_AWAY, FLOOR, CEIL, TRUNC = range(4)
CONVERSIONS = (A.EXPR_CAST, A.EXPR_ROUND, A.EXPR_FLOOR, A.EXPR_CEIL, A.EXPR_TRUNC)
DEC_LIMIT = 10 ** 38


def holds_conversion(e):
    return e.op in CONVERSIONS or any(holds_conversion(c) for c in e.children)


# ---- the five conversions on values ----

def to_f64(unscaled, scale):
    """the double nearest unscaled / 10^scale, ties to even"""
    return float(Fraction(unscaled, 10 ** scale))


def round_fraction(q, mode):
    """a Fraction -> an int by the mode"""
    if mode == FLOOR:
        return math.floor(q)
    if mode == CEIL:
        return math.ceil(q)
    t = math.trunc(q)
    if mode == HALF_AWAY and abs(q - t) >= Fraction(1, 2):
        t += 1 if q > 0 else -1
    return t


def rescale(unscaled, k, mode):
    """unscaled / 10^k to an integer by the mode"""
    return round_fraction(Fraction(unscaled, 10 ** k), mode)


def f64_to_dec(x, t):
    """round(x * 10^t) half away from zero of the double's exact value, or OVER: NaN, an infinity, |result| >= 10^38"""
    if math.isnan(x) or math.isinf(x):
        return OVER
    r = round_fraction(Fraction(x) * 10 ** t, HALF_AWAY)
    return OVER if abs(r) >= DEC_LIMIT else r


def f64_to_i64(x):
    if math.isnan(x) or math.isinf(x):
        return OVER
    r = math.trunc(x)
    return r if -2 ** 63 <= r < 2 ** 63 else OVER


def f64_round(x, mode):
    """C's round / floor / ceil / trunc: a double, the sign of a zero result the operand's (ceil(-0.5) is -0.0)"""
    x = float(x)
    if math.isnan(x) or math.isinf(x):
        return x
    if mode == HALF_AWAY:
        return math.copysign(float(abs(round_fraction(Fraction(x), HALF_AWAY))), x)
    return float({FLOOR: np.floor, CEIL: np.ceil, TRUNC: np.trunc}[mode](np.float64(x)))


# ---- types ----

def _col_type(name, schema):
    k = schema[name]
    return ("float", 0) if k == "float" else ("dec", k[1]) if isinstance(k, tuple) else ("int", 0)


def _int_literal(e):
    return e.op == A.EXPR_LITERAL and e.value_type == A.PV_INT64


def _meet(ea, ta, eb, tb):
    """the class of two operands that must be of one: a NULL takes its sibling's, an INT64 literal beside doubles is a double"""
    if ta is None:
        ta = tb
    if tb is None:
        tb = ta
    fa, fb = ta[0] == "float", tb[0] == "float"
    if fa != fb:
        lit = eb if fa else ea
        if not _int_literal(lit):
            raise AEM.Refused("mismatched", "a Float / Double operand beside an exact one")
        if int(float(lit.value)) != lit.value:
            raise AEM.Refused("invalid", "an INT64 literal that is not exact as a double")
        return "float"
    return "float" if fa else "dec" if "dec" in (ta[0], tb[0]) else "int"


def type_of(e, schema):
    """(class, scale) of node e, None for a NULL node; Refused as the compiler refuses"""
    op = e.op
    if op == A.EXPR_NULL:
        return None
    if op == A.EXPR_COLUMN:
        return _col_type(e.column, schema)
    if op == A.EXPR_LITERAL:
        return ("float", 0) if e.value_type == A.PV_FLOAT64 else ("dec", e.value[1]) if e.value_type == A.PV_DECIMAL128 else ("int", 0)
    kids = [type_of(c, schema) for c in e.children]
    if op in CDM.CONDITIONS:
        if op == A.EXPR_CMP:
            _meet(e.children[0], kids[0], e.children[1], kids[1])
        return ("cond", 0)
    if op == A.EXPR_CAST:
        return ("float", 0) if e.value_type == A.PV_FLOAT64 else ("dec", e.scale) if e.value_type == A.PV_DECIMAL128 else ("int", 0)
    if op == A.EXPR_ROUND:
        if kids[0][0] == "float":
            if e.scale != 0:
                raise AEM.Refused("unsupported", "round(double, n > 0)")
            return kids[0]
        return (kids[0][0], min(kids[0][1], e.scale))
    if op in (A.EXPR_FLOOR, A.EXPR_CEIL, A.EXPR_TRUNC):
        return (kids[0][0], 0)
    if op in (A.EXPR_NEG, A.EXPR_ABS):
        return kids[0]
    if op == A.EXPR_DATE_PART:
        if kids[0][0] == "float" or kids[0][1] != 0:
            raise AEM.Refused("mismatched", "a date part takes an integer")
        return ("int", 0)
    if op == A.EXPR_IF:
        ea, eb, ta, tb = e.children[1], e.children[2], kids[1], kids[2]
    else:
        ea, eb, ta, tb = e.children[0], e.children[1], kids[0], kids[1]
    k = _meet(ea, ta, eb, tb)
    if k == "float":
        if op in (A.EXPR_FLOOR_DIV, A.EXPR_MOD):
            raise AEM.Refused("mismatched", "// or % of doubles")
        return ("float", 0)
    sa = (ta or tb)[1]
    sb = (tb or ta)[1]
    if op == A.EXPR_MUL:
        s = sa + sb
    elif op == A.EXPR_DIV:
        DM.power_of(sa, sb, e.scale)
        k, s = "dec", DM.result_scale(sa, e.scale)
    elif op in (A.EXPR_FLOOR_DIV, A.EXPR_MOD):
        if sa or sb:
            raise AEM.Refused("mismatched", "// or % on a non-zero scale")
        s = 0
    else:
        s = max(sa, sb)
    if s > 38:
        raise AEM.Refused("unsupported", "scale %d" % s)
    return (k, s)


# ---- evaluation ----

def _as(v, t, e):
    """the state v of operand e brought to the operator's type t: an INT64 literal beside doubles is a double, an exact value goes
    to the operator's scale where the operator aligns (the caller decides)"""
    if v is None or v is OVER:
        return v
    if t[0] == "float" and isinstance(v, tuple):
        return np.float64(v[0])
    return v


def evaluate(e, schema, row):
    ev = lambda x: evaluate(x, schema, row)
    op = e.op
    if op == A.EXPR_NULL:
        return None
    if op == A.EXPR_COLUMN:
        v = row[e.column]
        if v is None:
            return None
        t = _col_type(e.column, schema)
        return np.float64(v) if t[0] == "float" else (int(v), t[1])
    if op == A.EXPR_LITERAL:
        if e.value_type == A.PV_FLOAT64:
            return np.float64(e.value)
        return (e.value[0], e.value[1]) if e.value_type == A.PV_DECIMAL128 else (e.value, 0)
    if op == A.EXPR_IS_NULL:
        a = ev(e.children[0])
        return OVER if a is OVER else a is None
    if op == A.EXPR_NOT:
        a = ev(e.children[0])
        return a if a is None or a is OVER else not a
    if op in (A.EXPR_AND, A.EXPR_OR):
        return CDM._kleene(op == A.EXPR_OR, ev(e.children[0]), ev(e.children[1]))
    t = type_of(e, schema)
    kids = [ev(c) for c in e.children]
    if op in CONVERSIONS:
        a, ta = kids[0], type_of(e.children[0], schema)
        if a is None or a is OVER:
            return a
        mode = {A.EXPR_ROUND: HALF_AWAY, A.EXPR_FLOOR: FLOOR, A.EXPR_CEIL: CEIL, A.EXPR_TRUNC: TRUNC}.get(op)
        if op == A.EXPR_CAST and t[0] == "float":
            return a if ta[0] == "float" else np.float64(to_f64(a[0], a[1]))
        if op == A.EXPR_CAST and t[0] == "dec":
            if ta[0] == "float":
                r = f64_to_dec(float(a), t[1])
                return OVER if r is OVER else (r, t[1])
            if t[1] >= a[1]:
                return CDM._to_scale(a, t[1])
            return (rescale(a[0], a[1] - t[1], HALF_AWAY), t[1])
        if op == A.EXPR_CAST:
            r = f64_to_i64(float(a)) if ta[0] == "float" else rescale(a[0], a[1], TRUNC)
            return OVER if r is OVER or not -2 ** 63 <= r < 2 ** 63 else (r, 0)
        if ta[0] == "float":
            return np.float64(f64_round(float(a), mode))
        if t[1] >= a[1]:
            return a
        return (rescale(a[0], a[1] - t[1], mode), t[1])
    if op == A.EXPR_IF:
        c, a, b = kids
        if c is OVER:
            return OVER
        chosen = _as(a if c is True else b, t, e.children[1 if c is True else 2])
        return chosen if t[0] == "float" else CDM._to_scale(chosen, t[1])
    if op == A.EXPR_COALESCE:
        chosen = _as(kids[1] if kids[0] is None else kids[0], t, e)
        return chosen if t[0] == "float" else CDM._to_scale(chosen, t[1])
    if op == A.EXPR_CMP:
        ta, tb = type_of(e.children[0], schema), type_of(e.children[1], schema)
        k = _meet(e.children[0], ta, e.children[1], tb)
        if k == "float":
            kids = [_as(v, ("float", 0), c) for v, c in zip(kids, e.children)]
        else:
            s = max(ta[1], tb[1])
            kids = [CDM._to_scale(v, s) for v in kids]
        first = CDM._first(*kids)
        if first != "go":
            return first
        return CDM._cmp(e.cmp, kids[0], kids[1]) if k == "float" else CDM._cmp(e.cmp, kids[0][0], kids[1][0])
    if t[0] == "float":
        kids = [_as(v, t, c) for v, c in zip(kids, e.children)]
        first = CDM._first(*kids)
        if first != "go":
            return first
        with np.errstate(all="ignore"):
            if op == A.EXPR_NEG:
                return -kids[0]
            if op == A.EXPR_ABS:
                return np.fabs(kids[0])
            if op == A.EXPR_DIV:
                return np.float64(DM.float_div(float(kids[0]), float(kids[1])))
            return kids[0] + kids[1] if op == A.EXPR_ADD else kids[0] - kids[1] if op == A.EXPR_SUB else kids[0] * kids[1]
    s = t[1]
    if op in (A.EXPR_ADD, A.EXPR_SUB):
        kids = [CDM._to_scale(k, s) for k in kids]
    first = CDM._first(*kids)
    if first != "go":
        return first
    a = kids[0][0]
    b = kids[1][0] if len(kids) > 1 else None
    if op == A.EXPR_DATE_PART:
        v = DPM.part_of(a, e.part)
    elif op == A.EXPR_DIV:
        v = DM.div_round(a, b, DM.power_of(kids[0][1], kids[1][1], e.scale))
    elif op in (A.EXPR_FLOOR_DIV, A.EXPR_MOD):
        v = DM.floor_div(a, b) if op == A.EXPR_FLOOR_DIV else DM.mod(a, b)
    else:
        v = {A.EXPR_ADD: lambda: a + b, A.EXPR_SUB: lambda: a - b, A.EXPR_MUL: lambda: a * b, A.EXPR_NEG: lambda: -a, A.EXPR_ABS: lambda: abs(a)}[op]()
    return OVER if v is None or not DM.fits(v) else (v, s)


# ---- the root decides the row ----

def computed_type(e, schema):
    CDM.check(e)
    k, s = type_of(e, schema)
    return (CM.FLOAT64, 0) if k == "float" else (CM.DEC128, s) if k == "dec" else (CM.INT64, 0)


def computed_value(e, schema, row):
    """(value, overflowed): (None, False) for NULL, (None, True) for an overflow of the expression or of the column's type"""
    kind, _ = computed_type(e, schema)
    v = evaluate(e, schema, row)
    if v is None or v is OVER:
        return None, v is OVER
    if kind == CM.FLOAT64:
        return float(v), False
    if (kind == CM.INT64 and not -2 ** 63 <= v[0] < 2 ** 63) or (kind == CM.DEC128 and abs(v[0]) >= DEC_LIMIT):
        return None, True
    return v[0], False


def computed_column(e, schema, rows):
    vals, over = [], 0
    for row in rows:
        v, o = computed_value(e, schema, row)
        vals.append(v)
        over += 1 if o else 0
    return vals, over


def agg_row(e, schema, row):
    """what an expression aggregate sees of a row: None (NULL), AEM.ROW_OVERFLOW, the unscaled int, or the float"""
    kind, _ = computed_type(e, schema)
    v = evaluate(e, schema, row)
    if v is None:
        return None
    if v is OVER:
        return AEM.ROW_OVERFLOW
    return float(v) if kind == CM.FLOAT64 else v[0]


def agg_scale(e, schema):
    return computed_type(e, schema)[1]


def filter_leaf(lhs, op, rhs, row, schema):
    """(True / False / None, overflowed) of lhs OP rhs on one row: the two sides meet as CMP's do.  NULL on either side comes
    first: UNKNOWN and not counted; else an overflow on either side: UNKNOWN and counted."""
    lhs, rhs = A.Expr._wrap(lhs), A.Expr._wrap(rhs)
    CDM.check(lhs)
    CDM.check(rhs)
    ta, tb = type_of(lhs, schema), type_of(rhs, schema)
    k = _meet(lhs, ta, rhs, tb)
    a, b = evaluate(lhs, schema, row), evaluate(rhs, schema, row)
    if a is None or b is None:
        return None, False
    if a is OVER or b is OVER:
        return None, True
    if k == "float":
        a, b = _as(a, ("float", 0), lhs), _as(b, ("float", 0), rhs)
        return CDM._cmp(P._CMP_OPS[op], a, b), False
    s = max(a[1], b[1])
    return CDM._cmp(P._CMP_OPS[op], a[0] * 10 ** (s - a[1]), b[0] * 10 ** (s - b[1])), False
