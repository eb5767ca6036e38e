"""The model of the row filter's expression leaf (include/orcgpu.h, ORCGPU_PRED_CMP_EXPR): lhs OP rhs over Python ints,
fractions.Fraction and floats.  Three-valued: True / False / None (UNKNOWN).  Plain Python, no library, no GPU.

A side is an orc_rust_amd.aggregate.Expr (pure data: op, children, column, value_type, value).  A schema maps a column name to
"int" (Byte .. Long, and Date as days), "float", or ("dec", scale).  A row maps a column name to an int (an int / Date value, or a
Decimal's unscaled value), a float, or None for NULL.

The rules, as the header states them:
  * the class -- INT, DEC, FLOAT -- is decided over both sides together; float and exact operands do not mix (ValueError here);
  * INT / DEC: every operation inside a side is exact in a signed 128-bit integer or the side has NO value (overflow): the leaf is
    UNKNOWN on that row, and the row is counted -- unless a column of either side is NULL, which comes first;
  * DEC: a + b and a - b bring the operand of the smaller scale to the larger one (times a power of ten, an operation like any
    other); a * b adds the scales; a scale past 38 is refused (ValueError here);
  * the comparison: INT as integers; DEC in exact rational order -- the side of the smaller scale times 10^d, and where that leaves
    128 bits the sign alone decides (a positive overflowing side is greater than any int128, a negative one smaller); FLOAT as
    IEEE doubles (a NaN on either side: everything but != is False; -0.0 == 0.0)."""
from fractions import Fraction

EXPR_COLUMN, EXPR_LITERAL, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG = range(6)
PV_INT64, PV_FLOAT64, PV_DECIMAL128 = 4, 6, 8
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
OVERFLOW = object()  # what a side is worth when an operation left 128 bits


def fits(v):
    return I128_MIN <= v <= I128_MAX


def _leaves(e):
    if not e.children:
        yield e
    for c in e.children:
        yield from _leaves(c)


def classify(sides, schema):
    """'int', 'dec' or 'float' for the two sides together; ValueError for a mix of float and exact operands; KeyError for a column
    the schema does not hold."""
    has_float = has_exact = has_dec = False
    for side in sides:
        for leaf in _leaves(side):
            if leaf.op == EXPR_COLUMN:
                t = schema[leaf.column]
                has_float |= t == "float"
                has_exact |= t != "float"
                has_dec |= isinstance(t, tuple)
    float_lit = any(leaf.op == EXPR_LITERAL and leaf.value_type == PV_FLOAT64 for s in sides for leaf in _leaves(s))
    dec_lit = any(leaf.op == EXPR_LITERAL and leaf.value_type == PV_DECIMAL128 for s in sides for leaf in _leaves(s))
    if (has_float and (has_exact or dec_lit)) or (float_lit and (has_exact or dec_lit)):
        raise ValueError("float and exact operands do not mix")
    return "float" if has_float or float_lit else "dec" if has_dec or dec_lit else "int"


def _exact(e, row, schema):
    """-> (value, scale), (OVERFLOW, scale), or None when a column is NULL.  The scales do not depend on the row."""
    if e.op == EXPR_COLUMN:
        t = schema[e.column]
        v = row[e.column]
        return None if v is None else (int(v), t[1] if isinstance(t, tuple) else 0)
    if e.op == EXPR_LITERAL:
        return (e.value[0], e.value[1]) if e.value_type == PV_DECIMAL128 else (int(e.value), 0)
    kids = [_exact(c, row, schema) for c in e.children]
    if any(k is None for k in kids):
        return None
    if e.op == EXPR_NEG:
        (a, sa), = kids
        r, s = (OVERFLOW if a is OVERFLOW else -a), sa
    else:
        (a, sa), (b, sb) = kids
        if e.op == EXPR_MUL:
            s = sa + sb
            r = OVERFLOW if a is OVERFLOW or b is OVERFLOW else a * b
        else:
            s = max(sa, sb)
            if s <= 38:  # (the operand of the smaller scale times a power of ten: an operation of its own)
                a = a if a is OVERFLOW else a * 10 ** (s - sa)
                b = b if b is OVERFLOW else b * 10 ** (s - sb)
                a = a if a is OVERFLOW or fits(a) else OVERFLOW
                b = b if b is OVERFLOW or fits(b) else OVERFLOW
            r = OVERFLOW if a is OVERFLOW or b is OVERFLOW else (a + b if e.op == EXPR_ADD else a - b)
    if s > 38:
        raise ValueError("a node of the expression has a scale of more than 38")
    return (r if r is OVERFLOW or fits(r) else OVERFLOW), s


def _float(e, row):
    if e.op == EXPR_COLUMN:
        v = row[e.column]
        return None if v is None else float(v)
    if e.op == EXPR_LITERAL:
        return float(e.value)
    kids = [_float(c, row) for c in e.children]
    if any(k is None for k in kids):
        return None
    if e.op == EXPR_NEG:
        return -kids[0]
    a, b = kids
    return a + b if e.op == EXPR_ADD else a - b if e.op == EXPR_SUB else a * b  # one IEEE double operation each


def _answer(op, lt, eq, gt):
    return {"=": eq, "!=": not eq, "<": lt, "<=": lt or eq, ">": gt, ">=": gt or eq}[op]


def compare_exact(op, a, sa, b, sb):
    """a * 10^-sa OP b * 10^-sb by the device's rule -- rescale the coarser side, decide an overflow by its sign -- checked against
    the exact rational order."""
    d = sb - sa
    if d >= 0:
        x = a * 10 ** d
        lt, gt = (x < b, x > b) if fits(x) else (a < 0, a > 0)
    else:
        y = b * 10 ** -d
        lt, gt = (a < y, a > y) if fits(y) else (b > 0, b < 0)
    fa, fb = Fraction(a, 10 ** sa), Fraction(b, 10 ** sb)
    assert (lt, gt) == (fa < fb, fa > fb), (a, sa, b, sb)
    return _answer(op, lt, not lt and not gt, gt)


def evaluate(lhs, op, rhs, row, schema):
    """-> (True / False / None, overflowed): the leaf on one row, and whether the row counts as an overflow evaluation."""
    cls = classify((lhs, rhs), schema)
    if cls == "float":
        a, b = _float(lhs, row), _float(rhs, row)
        if a is None or b is None:
            return None, False
        return _answer(op, a < b, a == b, a > b), False
    a, b = _exact(lhs, row, schema), _exact(rhs, row, schema)
    if a is None or b is None:
        return None, False
    if a[0] is OVERFLOW or b[0] is OVERFLOW:
        return None, True
    return compare_exact(op, a[0], a[1], b[0], b[1]), False


def kept(lhs, op, rhs, rows, schema):
    """-> (indices of the rows where the leaf is TRUE, the overflow count)"""
    out, over = [], 0
    for k, row in enumerate(rows):
        t, o = evaluate(lhs, op, rhs, row, schema)
        over += o
        if t is True:
            out.append(k)
    return out, over


def not3(t):
    return None if t is None else not t
