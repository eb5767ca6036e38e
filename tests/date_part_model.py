"""The model of the date part of an expression (include/orcgpu.h: DATE PARTS; orc_rust_amd.aggregate.year .. extract) in plain
Python ints, written without a look at the C text: inside one 400-year era the calendar is `datetime.date.fromordinal`'s, and a
day outside it is moved there by whole eras of 146097 days -- a multiple of 7, so the weekday moves with it -- and its year moved
back by 400 an era.  Proleptic Gregorian, astronomical year numbering.

Whole expressions go to the existing models unchanged: `lower` rewrites every date-part subtree of an expression into a synthetic
Int64 column that holds the model's value for the row at hand, and says whether one of them overflowed there -- its operand left
128 bits, or int32.  tests/computed_model.py, tests/agg_expr_model.py and tests/filter_model_expr.py then see columns, literals and
+ - * alone.  TEST INFRASTRUCTURE: nothing here is used by the product."""
import datetime

import agg_expr_model as AEM
import computed_model as CM
import filter_model_expr as FME
from orc_rust_amd import aggregate as A

ERA_DAYS, ERA_YEARS = 146097, 400
EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()
I32 = (-2 ** 31, 2 ** 31 - 1)
YEAR, QUARTER, MONTH, DAY, DAY_OF_WEEK, DAY_OF_YEAR = range(6)
assert A.DATE_PARTS == ("year", "quarter", "month", "day", "day_of_week", "day_of_year")


def civil(days):
    """days since 1970-01-01 (any int) -> (year, month, day, ISO weekday 1 .. 7, day of the year 1 .. 366)"""
    ordinal = days + EPOCH_ORDINAL  # 1 = 0001-01-01
    era = (ordinal - 1) // ERA_DAYS  # Python's floor: the eras before year 1 are negative
    d = datetime.date.fromordinal(ordinal - era * ERA_DAYS)  # in years 1 .. 400
    return d.year + era * ERA_YEARS, d.month, d.day, d.isoweekday(), d.timetuple().tm_yday


def part_of(days, part):
    """the field of the day, for days in int32; None outside it: the row overflows"""
    if not I32[0] <= days <= I32[1]:
        return None
    y, m, d, w, n = civil(days)
    return (y, (m - 1) // 3 + 1, m, d, w, n)[part]


def holds_date_part(e):
    return e.op == A.EXPR_DATE_PART or any(holds_date_part(c) for c in e.children)


def lower(e, row, prefix="__dp"):
    """-> (the expression with every date-part subtree replaced by a synthetic column, the row with those columns' values, whether
    a date part overflowed on this row).  A synthetic column is NULL where a column of its operand is; it is 0 where it overflowed."""
    out = dict(row)
    state = {"over": False, "n": 0}

    def walk(x):
        if x.op != A.EXPR_DATE_PART:
            if not x.children:
                return x
            return A.Expr(x.op, [walk(c) for c in x.children], x.column, x.value_type, x.value)
        operand = walk(x.children[0])
        name = "%s%d" % (prefix, state["n"])
        state["n"] += 1
        if any(out[leaf.column] is None for leaf in AEM.leaves(operand) if leaf.op == A.EXPR_COLUMN):
            out[name] = None
        else:
            try:
                v = part_of(AEM._exact(operand, out, {})[0], x.part)
            except AEM._Overflow:
                v = None
            state["over"] |= v is None
            out[name] = 0 if v is None else v
        return A.col(name)

    return walk(e), out, state["over"]


def _schema_with(schema, row):
    s = dict(schema)
    for name in row:
        if name not in s:
            s[name] = "int"
    return s


def _null(e, row):
    return any(row[leaf.column] is None for leaf in AEM.leaves(e) if leaf.op == A.EXPR_COLUMN)


def computed_value(e, schema, row):
    """computed_model.eval_value with date parts: (value, overflowed)"""
    if _null(e, row):
        return None, False
    low, row2, over = lower(e, row)
    if over:
        return None, True
    return CM.eval_value(low, _schema_with(schema, row2), row2)


def computed_type(e, schema):
    """computed_model.output_type with date parts (a date part is an integer column to the typing)"""
    low, row2, _ = lower(e, {leaf.column: 0 for leaf in AEM.leaves(e) if leaf.op == A.EXPR_COLUMN})
    return CM.output_type(low, _schema_with(schema, row2))


def computed_column(e, schema, rows):
    """computed_model.eval_column with date parts: (values, overflow count)"""
    vals, over = [], 0
    for row in rows:
        v, o = computed_value(e, schema, row)
        vals.append(v)
        over += 1 if o else 0
    return vals, over


def agg_row(e, schema, row):
    """agg_expr_model.eval_row with date parts: None (NULL), AEM.ROW_OVERFLOW, or the unscaled int"""
    if _null(e, row):
        return None
    low, row2, over = lower(e, row)
    if over:
        return AEM.ROW_OVERFLOW
    s2 = _schema_with(schema, row2)
    cls = AEM.classify(low, CM.families_of(s2))
    return AEM.eval_row(low, cls, row2, CM.scales_of(s2))


def filter_leaf(lhs, op, rhs, row, schema):
    """filter_model_expr.evaluate with date parts: (True / False / None, overflowed)"""
    lhs, rhs = A.Expr._wrap(lhs), A.Expr._wrap(rhs)  # (a plain number is a literal, as for Predicate.compare)
    if _null(lhs, row) or _null(rhs, row):
        return None, False
    l, row2, over_l = lower(lhs, row, "__dpl")
    r, row3, over_r = lower(rhs, row2, "__dpr")
    if over_l or over_r:
        return None, True
    s = {k: ("int" if v == "date" else v) for k, v in _schema_with(schema, row3).items()}
    return FME.evaluate(l, op, r, row3, s)
