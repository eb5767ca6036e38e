"""The model of the conditionals in an expression (include/orcgpu.h: CONDITIONALS; orc_rust_amd.aggregate.when / case / coalesce /
nullif / abs_): a tree evaluator over `None`, Python ints (`fractions.Fraction` inside the division model) and numpy `float64`,
written from the semantics, not from the C text.

Every operand is one of: NULL (None), OVER (the row's operation left 128 bits, divided by zero, ...), or a value -- for the INT /
DEC class the pair (unscaled int, scale), for the FLOAT class a numpy float64, for a condition True / False (None: UNKNOWN).

  arithmetic   NULL if an operand is NULL; otherwise OVER if an operand is OVER or the operation overflows.
  CMP          the same, UNKNOWN for NULL; exact after the smaller scale is brought to the larger (which can overflow that side);
               doubles by IEEE.
  IS_NULL      never UNKNOWN; OVER of an operand that overflowed.
  AND, OR      a known FALSE decides AND and a known TRUE decides OR whatever the other side is; otherwise OVER before UNKNOWN.
  IF           the chosen branch's state (FALSE and UNKNOWN choose `otherwise`); a condition that is OVER makes the IF OVER.
  COALESCE     a unless a is NULL, then b.
  the root     decides the row: see computed_value, agg_row and filter_leaf.

The nodes below are the existing models': division is tests/div_model.py (div_round, floor_div, mod, float_div, the scale rule), a
date part tests/date_part_model.py (part_of).  TEST INFRASTRUCTURE: nothing here is used by the product."""
import numpy as np

import agg_expr_model as AEM
import computed_model as CM
import date_part_model as DPM
import div_model as DM
from orc_rust_amd import aggregate as A
from orc_rust_amd import predicate as P


class _Over:
    def __repr__(self):
        return "OVER"


OVER = _Over()
I64 = (-2 ** 63, 2 ** 63 - 1)
CONDITIONS = (A.EXPR_CMP, A.EXPR_IS_NULL, A.EXPR_AND, A.EXPR_OR, A.EXPR_NOT)
CONDITIONALS = tuple(range(A.EXPR_IF, A.EXPR_NOT + 1))


def holds_conditional(e):
    return e.op in CONDITIONALS or any(holds_conditional(c) for c in e.children)


def check(e, want_cond=False, null_ok=False):
    """numbers where numbers are wanted, conditions where conditions are; a NULL only as a value operand of IF / COALESCE whose
    sibling is no NULL: Refused('invalid') otherwise"""
    if (e.op in CONDITIONS) != want_cond:
        raise AEM.Refused("invalid", "%r where a %s is wanted" % (e, "condition" if want_cond else "number"))
    if e.op == A.EXPR_NULL and not null_ok:
        raise AEM.Refused("invalid", "NULL outside the value operands of IF / COALESCE")
    for k, c in enumerate(e.children):
        if e.op == A.EXPR_IF:
            check(c, k == 0, k != 0 and e.children[3 - k].op != A.EXPR_NULL)
        elif e.op == A.EXPR_COALESCE:
            check(c, False, e.children[1 - k].op != A.EXPR_NULL)
        else:
            check(c, e.op in (A.EXPR_AND, A.EXPR_OR, A.EXPR_NOT), False)


def classify(exprs, schema):
    """'float' | 'dec' | 'int' of the expressions typed together, or Refused as + refuses a Float / Double beside an exact operand"""
    leaves = [x for e in exprs for x in AEM.leaves(e)]
    cols = [x for x in leaves if x.op == A.EXPR_COLUMN]
    lits = [x for x in leaves if x.op == A.EXPR_LITERAL]
    fam = lambda c: "float" if schema[c.column] == "float" else "dec" if isinstance(schema[c.column], tuple) else "int"
    has_float, has_exact = any(fam(c) == "float" for c in cols), any(fam(c) != "float" for c in cols)
    if has_float and has_exact:
        raise AEM.Refused("mismatched", "float and exact columns")
    if has_exact and any(x.value_type == A.PV_FLOAT64 for x in lits):
        raise AEM.Refused("mismatched", "FLOAT64 literal")
    if has_float and any(x.value_type == A.PV_DECIMAL128 for x in lits):
        raise AEM.Refused("mismatched", "DECIMAL128 literal")
    if has_float or (not cols and any(x.value_type == A.PV_FLOAT64 for x in lits)):
        return "float"

    def has_div(e):
        return e.op == A.EXPR_DIV or any(has_div(c) for c in e.children)
    if any(fam(c) == "dec" for c in cols) or any(x.value_type == A.PV_DECIMAL128 for x in lits) or any(has_div(e) for e in exprs):
        return "dec"
    return "int"


def scale_of(e, schema):
    """the scale of a number node of the INT / DEC class (None: a NULL node, which takes its sibling's)"""
    if e.op == A.EXPR_COLUMN:
        return schema[e.column][1] if isinstance(schema[e.column], tuple) else 0
    if e.op == A.EXPR_LITERAL:
        return e.value[1] if e.value_type == A.PV_DECIMAL128 else 0
    if e.op == A.EXPR_NULL:
        return None
    if e.op in CONDITIONS or e.op in (A.EXPR_DATE_PART, A.EXPR_FLOOR_DIV, A.EXPR_MOD):
        return 0
    kids = [scale_of(c, schema) for c in e.children]
    if e.op == A.EXPR_MUL:
        s = kids[0] + kids[1]
    elif e.op == A.EXPR_DIV:
        DM.power_of(kids[0], kids[1], e.scale)
        s = DM.result_scale(kids[0], e.scale)
    elif e.op == A.EXPR_IF:
        s = max(k for k in kids[1:] if k is not None)
    else:  # + -, unary -, ABS, COALESCE
        s = max(k for k in kids if k is not None)
    if s > 38:
        raise AEM.Refused("unsupported", "scale %d" % s)
    return s


def _to_scale(v, s):
    """the value state v = (unscaled, scale) at scale s: OVER when the product leaves 128 bits; NULL and OVER pass"""
    if v is None or v is OVER:
        return v
    u = v[0] * 10 ** (s - v[1])
    return (u, s) if DM.fits(u) else OVER


def _first(*states):
    """NULL first, then OVER: what arithmetic makes of its operands' states, or 'go' when all are values"""
    if any(s is None for s in states):
        return None
    if any(s is OVER for s in states):
        return OVER
    return "go"


def _kleene(is_or, a, b):
    if a is is_or or b is is_or:  # (True / False are singletons: a known TRUE under OR, a known FALSE under AND)
        return is_or
    if a is OVER or b is OVER:
        return OVER
    if a is None or b is None:
        return None
    return not is_or


def _cmp(op, a, b):
    return bool({P.EQ: a == b, P.NE: a != b, P.LT: a < b, P.LE: a <= b, P.GT: a > b, P.GE: a >= b}[op])


def evaluate(e, schema, row, floating):
    """the state of node e on the row: None, OVER, (unscaled, scale) / numpy.float64, or True / False"""
    ev = lambda x: evaluate(x, schema, row, floating)
    op = e.op
    if op == A.EXPR_NULL:
        return None
    if op == A.EXPR_COLUMN:
        v = row[e.column]
        if v is None:
            return None
        return np.float64(v) if floating else (int(v), scale_of(e, schema))
    if op == A.EXPR_LITERAL:
        if floating:
            return np.float64(e.value)
        return (e.value[0], e.value[1]) if e.value_type == A.PV_DECIMAL128 else (e.value, 0)
    if op == A.EXPR_IS_NULL:
        a = ev(e.children[0])
        return OVER if a is OVER else a is None
    if op == A.EXPR_NOT:
        a = ev(e.children[0])
        return a if a is None or a is OVER else not a
    if op in (A.EXPR_AND, A.EXPR_OR):
        return _kleene(op == A.EXPR_OR, ev(e.children[0]), ev(e.children[1]))
    if op == A.EXPR_IF:
        c, a, b = (ev(x) for x in e.children)  # (both branches are evaluated: nothing of the other one may show)
        if c is OVER:
            return OVER
        chosen = a if c is True else b
        return chosen if floating else _to_scale(chosen, scale_of(e, schema))
    if op == A.EXPR_COALESCE:
        a, b = ev(e.children[0]), ev(e.children[1])
        chosen = b if a is None else a
        return chosen if floating else _to_scale(chosen, scale_of(e, schema))
    kids = [ev(c) for c in e.children]
    if op == A.EXPR_CMP:
        if not floating:
            s = max(scale_of(c, schema) for c in e.children)
            kids = [_to_scale(k, s) for k in kids]
        first = _first(*kids)
        if first != "go":
            return first
        return _cmp(e.cmp, kids[0], kids[1]) if floating else _cmp(e.cmp, kids[0][0], kids[1][0])
    if floating:
        first = _first(*kids)
        if first != "go":
            return first
        with np.errstate(all="ignore"):
            if op == A.EXPR_NEG:
                return -kids[0]
            if op == A.EXPR_ABS:
                return np.fabs(kids[0])
            if op == A.EXPR_DIV:
                return np.float64(DM.float_div(float(kids[0]), float(kids[1])))
            if op in (A.EXPR_FLOOR_DIV, A.EXPR_MOD, A.EXPR_DATE_PART):
                raise AEM.Refused("mismatched", "an integer operator in a Float / Double expression")
            return kids[0] + kids[1] if op == A.EXPR_ADD else kids[0] - kids[1] if op == A.EXPR_SUB else kids[0] * kids[1]
    s = scale_of(e, schema)
    if op in (A.EXPR_ADD, A.EXPR_SUB):
        kids = [_to_scale(k, s) for k in kids]
    first = _first(*kids)
    if first != "go":
        return first
    a = kids[0][0]
    b = kids[1][0] if len(kids) > 1 else None
    if op == A.EXPR_DATE_PART:
        if kids[0][1] != 0:
            raise AEM.Refused("mismatched", "a date part of a non-zero scale")
        v = DPM.part_of(a, e.part)
    elif op == A.EXPR_DIV:
        v = DM.div_round(a, b, DM.power_of(kids[0][1], kids[1][1], e.scale))
    elif op in (A.EXPR_FLOOR_DIV, A.EXPR_MOD):
        if kids[0][1] or kids[1][1]:
            raise AEM.Refused("mismatched", "// or % on a non-zero scale")
        v = DM.floor_div(a, b) if op == A.EXPR_FLOOR_DIV else DM.mod(a, b)
    else:
        v = {A.EXPR_ADD: lambda: a + b, A.EXPR_SUB: lambda: a - b, A.EXPR_MUL: lambda: a * b, A.EXPR_NEG: lambda: -a, A.EXPR_ABS: lambda: abs(a)}[op]()
    return OVER if v is None or not DM.fits(v) else (v, s)


def computed_type(e, schema):
    check(e)
    cls = classify([e], schema)
    return (CM.FLOAT64, 0) if cls == "float" else (CM.DEC128, scale_of(e, schema)) if cls == "dec" else (CM.INT64, 0)


def computed_value(e, schema, row):
    """(value, overflowed) of a computed column on one row: (None, False) for NULL, (None, True) for an overflow -- of the
    expression, or of the column's type: an Int64 column holds int64, a Decimal128 column |v| < 10^38"""
    kind, _ = computed_type(e, schema)
    v = evaluate(e, schema, row, kind == CM.FLOAT64)
    if v is None or v is OVER:
        return None, v is OVER
    if kind == CM.FLOAT64:
        return float(v), False
    if (kind == CM.INT64 and not I64[0] <= v[0] <= I64[1]) or abs(v[0]) >= CM.DEC_LIMIT and kind == CM.DEC128:
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
    """what an expression aggregate sees of a row: None (NULL: it contributes nothing), AEM.ROW_OVERFLOW, the unscaled int, or
    the float"""
    kind, _ = computed_type(e, schema)
    v = evaluate(e, schema, row, kind == CM.FLOAT64)
    if v is None:
        return None
    if v is OVER:
        return AEM.ROW_OVERFLOW
    return float(v) if kind == CM.FLOAT64 else v[0]


def agg_scale(e, schema):
    return computed_type(e, schema)[1]


def filter_leaf(lhs, op, rhs, row, schema):
    """(True / False / None, overflowed) of lhs OP rhs on one row, the two sides typed together.  NULL on either side comes first:
    UNKNOWN and not counted; else an overflow on either side: UNKNOWN and counted."""
    lhs, rhs = A.Expr._wrap(lhs), A.Expr._wrap(rhs)
    check(lhs)
    check(rhs)
    floating = classify([lhs, rhs], schema) == "float"
    a, b = evaluate(lhs, schema, row, floating), evaluate(rhs, schema, row, floating)
    if a is None or b is None:
        return None, False
    if a is OVER or b is OVER:
        return None, True
    if floating:
        return _cmp(P._CMP_OPS[op], a, b), False
    s = max(a[1], b[1])  # (the leaf's own alignment is in 256 bits: it does not overflow)
    return _cmp(P._CMP_OPS[op], a[0] * 10 ** (s - a[1]), b[0] * 10 ** (s - b[1])), False
