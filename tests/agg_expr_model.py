"""The model of SUM / AVG over arithmetic expressions (include/orcgpu.h, orcgpu_result_aggregate_exprs) in plain Python: Python
ints for every INT / DEC value, `fractions.Fraction` and `decimal` at precision 80 for AVG, Python floats in the given operation
order for FLOAT.  An expression is an orc_rust_amd.aggregate.Expr; a column is described by its family ('int', 'decimal', 'float')
and scale, as tests/agg_model.py's column_values gives them.  TEST INFRASTRUCTURE: nothing here is used by the product."""
import decimal
import fractions
import math

import agg_model as AM
from orc_rust_amd import aggregate as A

EXACT = decimal.Context(prec=80)
I128 = (-2 ** 127, 2 ** 127 - 1)
ROW_OVERFLOW = "row overflow"   # a row one of whose operations left 128 bits: it counts, its value is left out, the flag is set
INT, DEC, FLOAT = "int", "dec", "float"


class Refused(Exception):
    """what the plan compiler refuses: .status is 'mismatched' | 'unsupported' | 'invalid'"""

    def __init__(self, status, why):
        Exception.__init__(self, why)
        self.status = status


def leaves(e):
    if not e.children:
        return [e]
    return [x for c in e.children for x in leaves(c)]


def classify(e, families):
    """families: column name -> 'int' | 'decimal' | 'float' | anything else.  -> INT | DEC | FLOAT, or Refused"""
    if e.node_count() > A.EXPR_MAX_NODES:
        raise Refused("invalid", "more than 32 nodes")
    cols = [x for x in leaves(e) if x.op == A.EXPR_COLUMN]
    lits = [x for x in leaves(e) if x.op == A.EXPR_LITERAL]
    for c in cols:
        if c.column not in families:
            raise Refused("invalid", "unknown column %s" % c.column)
    if not cols:
        raise Refused("invalid", "no column")
    for c in cols:
        if families[c.column] not in ("int", "decimal", "float"):
            raise Refused("mismatched", c.column)
    has_float = any(families[c.column] == "float" for c in cols)
    has_exact = any(families[c.column] != "float" for c in cols)
    if has_float and has_exact:
        raise Refused("mismatched", "float and exact columns")
    if has_exact and any(x.value_type == A.PV_FLOAT64 for x in lits):
        raise Refused("mismatched", "FLOAT64 literal")
    if has_float and any(x.value_type == A.PV_DECIMAL128 for x in lits):
        raise Refused("mismatched", "DECIMAL128 literal")
    if has_float:
        for x in lits:
            if x.value_type == A.PV_INT64 and int(float(x.value)) != x.value:
                raise Refused("invalid", "inexact INT64 literal")
        return FLOAT
    if any(families[c.column] == "decimal" for c in cols) or any(x.value_type == A.PV_DECIMAL128 for x in lits):
        return DEC
    return INT


def scale_of(e, scales):
    """the Decimal scale of a node (Refused('unsupported') past 38); scales: column name -> scale (0 for integers)"""
    if e.op == A.EXPR_COLUMN:
        s = scales.get(e.column, 0)
    elif e.op == A.EXPR_LITERAL:
        s = e.value[1] if e.value_type == A.PV_DECIMAL128 else 0
    elif e.op == A.EXPR_MUL:
        s = scale_of(e.children[0], scales) + scale_of(e.children[1], scales)
    else:
        s = max(scale_of(c, scales) for c in e.children)
    if s > 38:
        raise Refused("unsupported", "scale %d" % s)
    return s


def slots(e):
    """operand slots when the child that needs more goes first, literal-only subtrees counting as one literal.  The "times 10^k"
    that aligns the scales of a Decimal a + b is unary: it needs what its operand needs, so the scales do not show here."""
    if not e.children or all(x.op == A.EXPR_LITERAL for x in leaves(e)):
        return 1
    if len(e.children) == 1:
        return slots(e.children[0])
    a, b = slots(e.children[0]), slots(e.children[1])
    return a + 1 if a == b else max(a, b)


class _Overflow(Exception):
    pass


def _fit(v):
    if not I128[0] <= v <= I128[1]:
        raise _Overflow()
    return v


def _exact(e, row, scales):
    """(unscaled value, scale) of a node of the INT / DEC class; every operation's exact result must fit 128 bits"""
    if e.op == A.EXPR_COLUMN:
        return row[e.column], scales.get(e.column, 0)
    if e.op == A.EXPR_LITERAL:
        return (e.value[0], e.value[1]) if e.value_type == A.PV_DECIMAL128 else (e.value, 0)
    a, sa = _exact(e.children[0], row, scales)
    if e.op == A.EXPR_NEG:
        return _fit(-a), sa
    b, sb = _exact(e.children[1], row, scales)
    if e.op == A.EXPR_MUL:
        return _fit(a * b), sa + sb
    s = max(sa, sb)
    if sa < s:
        a = _fit(a * 10 ** (s - sa))
    if sb < s:
        b = _fit(b * 10 ** (s - sb))
    return _fit(a + b if e.op == A.EXPR_ADD else a - b), s


def _float(e, row):
    if e.op == A.EXPR_COLUMN:
        return row[e.column]
    if e.op == A.EXPR_LITERAL:
        return float(e.value)
    a = _float(e.children[0], row)
    if e.op == A.EXPR_NEG:
        return -a
    b = _float(e.children[1], row)
    return a + b if e.op == A.EXPR_ADD else a - b if e.op == A.EXPR_SUB else a * b


def eval_row(e, cls, row, scales):
    """None when a column of the expression is NULL in the row; ROW_OVERFLOW; else the unscaled int, or the float"""
    if any(row[x.column] is None for x in leaves(e) if x.op == A.EXPR_COLUMN):
        return None
    if cls == FLOAT:
        return _float(e, row)
    try:
        return _exact(e, row, scales)[0]
    except _Overflow:
        return ROW_OVERFLOW


def avg_decimal(total, count, scale):
    """(unscaled, scale) of total / count at min(scale + 4, 38), half away from zero -- through Fraction, never through a float"""
    rs = min(scale + 4, 38)
    q = fractions.Fraction(total * 10 ** (rs - scale), count)
    n = abs(q)
    r = n.numerator // n.denominator
    if (n - r) * 2 >= 1:
        r += 1
    return (-r if q < 0 else r), rs


def avg_int(total, count):
    """the double nearest to total / count, ties to even: Python's true division of ints is correctly rounded"""
    return total / count


def table_info(table, names):
    """(values per column, families, scales) for the columns `names` of a pyarrow table"""
    vals, fam, sc = {}, {}, {}
    for n in names:
        v, f, s = AM.column_values(table, n)
        vals[n], fam[n], sc[n] = v, f, s
    return vals, fam, sc


def aggregate_expr(table, spec, keep):
    """What Agg.sum(expr) / Agg.avg(expr) / Agg.avg(column) give over the kept rows of `table`: int, decimal.Decimal, float, None, or
    AM.OVERFLOW.  float_terms(...) gives the doubles a FLOAT sum adds up."""
    if spec.op == A.AVG:
        e = A.col(spec.column)
    else:
        e = spec.expr
    names = sorted({x.column for x in leaves(e) if x.op == A.EXPR_COLUMN})
    vals, fam, sc = table_info(table, names)
    cls = classify(e, fam)
    root_scale = scale_of(e, sc) if cls == DEC else 0
    rows = []
    for i in range(table.num_rows):
        if keep[i]:
            v = eval_row(e, cls, {n: vals[n][i] for n in names}, sc)
            if v is not None:
                rows.append(v)
    avg = spec.op in (A.AVG, A.AVG_EXPR)
    if not rows:
        return None
    if cls == FLOAT:
        s = AM.float_sum(rows)
        return s / len(rows) if avg else s
    if any(v == ROW_OVERFLOW for v in rows):
        return AM.OVERFLOW
    total = sum(rows)
    if cls == INT:
        if not I128[0] <= total <= I128[1]:
            return AM.OVERFLOW
        return avg_int(total, len(rows)) if avg else total
    if abs(total) >= 10 ** 38:
        return AM.OVERFLOW
    if avg:
        total, root_scale = avg_decimal(total, len(rows), root_scale)
        if abs(total) >= 10 ** 38:
            return AM.OVERFLOW
    return decimal.Decimal(total).scaleb(-root_scale, EXACT)


def float_terms(table, spec, keep):
    e = A.col(spec.column) if spec.op == A.AVG else spec.expr
    names = sorted({x.column for x in leaves(e) if x.op == A.EXPR_COLUMN})
    vals, fam, sc = table_info(table, names)
    out = []
    for i in range(table.num_rows):
        if keep[i]:
            v = eval_row(e, FLOAT, {n: vals[n][i] for n in names}, sc)
            if v is not None:
                out.append(v)
    return out


def tokens(e):
    """the expression in the pre-order token form tests/hostcheck/agg_expr_check.cpp reads"""
    if e.op == A.EXPR_COLUMN:
        return ["c:" + e.column]
    if e.op == A.EXPR_LITERAL:
        if e.value_type == A.PV_DECIMAL128:
            return ["d:%d:%d" % e.value]
        return ["f:" + float(e.value).hex()] if e.value_type == A.PV_FLOAT64 else ["i:%d" % e.value]
    head = {A.EXPR_ADD: "+", A.EXPR_SUB: "-", A.EXPR_MUL: "*", A.EXPR_NEG: "neg"}[e.op]
    return [head] + [t for c in e.children for t in tokens(c)]


def is_finite(x):
    return not (math.isnan(x) or math.isinf(x))
