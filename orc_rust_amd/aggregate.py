"""Aggregates over the kept rows, reduced on the GPU (include/orcgpu.h: orcgpu_result_aggregate, orcgpu_reader_set_aggregates,
orcgpu_reader_aggregate): the specs a caller writes, their C form, and the Python values the results become.

    from orc_rust_amd.aggregate import Agg
    total, = ArrowReaderBuilder.try_new("lineitem.orc").with_projection([...]).with_row_filter(q6).aggregate(
        [Agg.sum_product("l_extendedprice", "l_discount")])          # a decimal.Decimal

An aggregate's argument may be an arithmetic expression over columns and literals, evaluated exactly per kept row on the GPU
(orcgpu_result_aggregate_exprs): `col(name)` and `lit(v)` build an Expr, `+ - *` and unary `-` combine them, plain Python numbers
on either side are wrapped; `/` (and `divide(a, b, scale=n)` to choose a Decimal quotient's scale), `//` and `%` divide -- exactly,
a zero divisor an overflow of the row, `//` and `%` on integers with Python's floor rule; `year(e)`, `quarter(e)`, `month(e)`, `day(e)`, `day_of_week(e)`, `day_of_year(e)` and `extract(part, e)`
take a calendar field of a Date (or of any integer expression of days since 1970-01-01); `when(cond, a, b)`, `case([(c1, a), ...],
otherwise)`, `coalesce(a, b, ...)`, `nullif(a, b)` and `abs(e)` choose per row -- SQL's CASE WHEN, COALESCE, NULLIF and ABS, with NULL
and overflow tracked per operand, so that the branch not taken is never seen: `when(col("b").ne(0), col("a") / col("b"), 0)`.
`cast(e, "int64")`, `cast(e, "float64")` and `cast(e, decimal_(scale))` convert between the classes (the Decimal target is spelled
`decimal_` in this module, where `decimal` is the standard library's; the package exports it as `orc_rust_amd.decimal` too) -- a Decimal beside a Double needs
one: `cast("l_quantity", "float64") * col("weight")` --, and `round_(e, digits)`, `floor(e)`, `ceil(e)`, `trunc(e)` (also Python's
`round(expr, 2)`, `math.floor(expr)`, `math.ceil(expr)`, `math.trunc(expr)`) round inside a class: a Decimal half away from zero to
`digits` places, or to the integer below, above or toward zero; a double by C's round / floor / ceil / trunc.  Exact and
deterministic: a cast to float64 is the nearest double of the exact value, a cast to int64 truncates toward zero, and a value the
target cannot hold overflows the row.
TPC-H Q1 whole:

    from orc_rust_amd.aggregate import Agg, col
    price, disc, tax = col("l_extendedprice"), col("l_discount"), col("l_tax")
    q1 = builder.aggregate([Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum(price * (1 - disc)), Agg.sum(price * (1 - disc) * (1 + tax)),
                            Agg.avg("l_quantity"), Agg.avg("l_extendedprice"), Agg.avg("l_discount"), Agg.count_rows()],
                           group_by=["l_returnflag", "l_linestatus"])

Pure plumbing: nothing is computed here, and every argument is checked before anything reaches the GPU."""
import ctypes as C
import decimal

from .predicate import _CMP_SIGNS, Predicate, PredicateNode

COUNT_ROWS, COUNT, SUM, MIN, MAX, SUM_PRODUCT, SUM_EXPR, AVG, AVG_EXPR = range(9)  # ORCGPU_AGG_OP_*
EXPR_COLUMN, EXPR_LITERAL, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG = range(6)  # ORCGPU_AGG_EXPR_*
EXPR_DATE_PART = 16  # ORCGPU_AGG_EXPR_DATE_PART (6 .. 15 are unknown nodes): one child, the part in the node's `i`
EXPR_DIV, EXPR_FLOOR_DIV, EXPR_MOD = 17, 18, 19  # ORCGPU_AGG_EXPR_DIV / _FLOOR_DIV / _MOD: two children; DIV: the result scale, or -1, in `i`
# ORCGPU_AGG_EXPR_IF .. _NOT (20 is an unknown node): the conditionals.  IF (condition, then, otherwise), COALESCE (2), ABS (1) and NULL
# (0 children) are numbers; CMP (2; the comparison EQ .. GE in `i`), IS_NULL (1), AND, OR (2) and NOT (1) are conditions
EXPR_IF, EXPR_COALESCE, EXPR_ABS, EXPR_NULL, EXPR_CMP, EXPR_IS_NULL, EXPR_AND, EXPR_OR, EXPR_NOT = range(21, 30)
_CONDITIONS = (EXPR_CMP, EXPR_IS_NULL, EXPR_AND, EXPR_OR, EXPR_NOT)
# ORCGPU_AGG_EXPR_CAST .. _TRUNC: the conversions, one child each.  CAST: the target in the node's value_type (PV_INT64 / PV_FLOAT64 /
# PV_DECIMAL128) and, for a Decimal target, the scale in `i`; ROUND: the digits in `i`
EXPR_CAST, EXPR_ROUND, EXPR_FLOOR, EXPR_CEIL, EXPR_TRUNC = range(30, 35)
DATE_PARTS = ("year", "quarter", "month", "day", "day_of_week", "day_of_year")  # ORCGPU_DATE_PART_*, by number
PV_INT64, PV_FLOAT64, PV_DECIMAL128 = 4, 6, 8  # ORCGPU_PV_* of an expression's literals
EXPR_MAX_NODES, EXPR_MAX_DEPTH = 32, 4  # ORCGPU_AGG_EXPR_MAX_*
KIND_U64, KIND_I128, KIND_DEC128, KIND_F64, KIND_I64 = range(5)  # ORCGPU_AGG_KIND_*
AGG_MAX = 64  # ORCGPU_AGG_MAX
GROUP_KEY_I64, GROUP_KEY_DEC128, GROUP_KEY_BOOL, GROUP_KEY_STRING = range(4)  # ORCGPU_GROUP_KEY_*
GROUP_MAX_KEYS, GROUP_MAX, GROUP_MAX_TOTAL, GROUP_KEY_BYTES = 4, 256, 65536, 64  # ORCGPU_GROUP_*
GROUP_LIMIT_MAX, GROUP_TOTAL_LIMIT_MAX = 1 << 20, 1 << 24  # ORCGPU_GROUP_LIMIT_MAX, ORCGPU_GROUP_TOTAL_LIMIT_MAX
_NAMES = ("count_rows", "count", "sum", "min", "max", "sum_product", "sum", "avg", "avg")
TS_UNITS = ("s", "ms", "us", "ns")


class AggSpec(C.Structure):
    _fields_ = [("op", C.c_uint32), ("column", C.c_char_p), ("column2", C.c_char_p)]


class AggExprNode(C.Structure):
    _fields_ = [("op", C.c_uint32), ("column", C.c_char_p), ("value_type", C.c_int32), ("i", C.c_int64), ("f", C.c_double), ("s", C.c_char_p),
                ("s_len", C.c_uint64)]


class AggExpr(C.Structure):
    _fields_ = [("nodes", C.POINTER(AggExprNode)), ("n_nodes", C.c_uint32)]


class AggFilter(C.Structure):
    _fields_ = [("nodes", C.POINTER(PredicateNode)), ("n_nodes", C.c_uint32)]


class AggValue(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("is_null", C.c_uint32), ("overflow", C.c_uint32), ("scale_or_unit", C.c_int32), ("w", C.c_uint64 * 3),
                ("f", C.c_double)]


class GroupKey(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("is_null", C.c_uint32), ("scale_or_unit", C.c_int32), ("len", C.c_uint32), ("w", C.c_uint64 * 2),
                ("bytes", C.c_uint8 * GROUP_KEY_BYTES)]


def _column(what, name):
    if not isinstance(name, str):
        raise TypeError("%s: a column name must be a str, not %s" % (what, type(name).__name__))
    if not name:
        raise ValueError("%s: an empty column name" % what)
    return name


class Expr:
    """An arithmetic expression over columns and literals: built by col() and lit(), combined with + - * / // % and unary -."""

    def __init__(self, op, children=(), column=None, value_type=None, value=None, part=None, scale=None, cmp=None):
        self.op, self.children, self.column, self.value_type, self.value = op, tuple(children), column, value_type, value
        self.part = part  # EXPR_DATE_PART: the index into DATE_PARTS
        self.scale = scale  # EXPR_DIV: the scale of an exact quotient the caller chose (divide), None: the default rule
        self.cmp = cmp  # EXPR_CMP: predicate.EQ .. GE
        # (EXPR_CAST: value_type is the target and `scale` a Decimal target's scale; EXPR_ROUND: `scale` holds the digits)

    @staticmethod
    def _wrap(x):
        return x if isinstance(x, Expr) else lit(x)

    def __abs__(self):
        return abs_(self)

    def __round__(self, digits=None):
        return round_(self, 0 if digits is None else digits)

    def __floor__(self):
        return floor(self)

    def __ceil__(self):
        return ceil(self)

    def __trunc__(self):
        return trunc(self)

    def __add__(self, other):
        return Expr(EXPR_ADD, (self, Expr._wrap(other)))

    def __radd__(self, other):
        return Expr(EXPR_ADD, (Expr._wrap(other), self))

    def __sub__(self, other):
        return Expr(EXPR_SUB, (self, Expr._wrap(other)))

    def __rsub__(self, other):
        return Expr(EXPR_SUB, (Expr._wrap(other), self))

    def __mul__(self, other):
        return Expr(EXPR_MUL, (self, Expr._wrap(other)))

    def __rmul__(self, other):
        return Expr(EXPR_MUL, (Expr._wrap(other), self))

    def __truediv__(self, other):
        return Expr(EXPR_DIV, (self, Expr._wrap(other)))

    def __rtruediv__(self, other):
        return Expr(EXPR_DIV, (Expr._wrap(other), self))

    def __floordiv__(self, other):
        return Expr(EXPR_FLOOR_DIV, (self, Expr._wrap(other)))

    def __rfloordiv__(self, other):
        return Expr(EXPR_FLOOR_DIV, (Expr._wrap(other), self))

    def __mod__(self, other):
        return Expr(EXPR_MOD, (self, Expr._wrap(other)))

    def __rmod__(self, other):
        return Expr(EXPR_MOD, (Expr._wrap(other), self))

    def __neg__(self):
        return Expr(EXPR_NEG, (self,))

    # A comparison of two expressions is a row filter's leaf (Predicate.compare).  `==` and `!=` stay what they are -- identity,
    # with the hash that goes with it: .eq(x) / .ne(x) build those two.
    def __lt__(self, other):
        return Predicate.compare(self, "<", other)

    def __le__(self, other):
        return Predicate.compare(self, "<=", other)

    def __gt__(self, other):
        return Predicate.compare(self, ">", other)

    def __ge__(self, other):
        return Predicate.compare(self, ">=", other)

    def eq(self, other):
        return Predicate.compare(self, "=", other)

    def ne(self, other):
        return Predicate.compare(self, "!=", other)

    def __repr__(self):
        if self.op == EXPR_COLUMN:
            return "col(%r)" % self.column
        if self.op == EXPR_LITERAL:
            if self.value_type == PV_DECIMAL128:
                return "lit(Decimal('%s'))" % decimal.Decimal(self.value[0]).scaleb(-self.value[1], _WIDE)
            return "lit(%r)" % (self.value,)
        if self.op == EXPR_NEG:
            return "(-%r)" % (self.children[0],)
        if self.op == EXPR_DATE_PART:
            return "%s(%r)" % (DATE_PARTS[self.part], self.children[0])
        if self.op == EXPR_DIV and self.scale is not None:
            return "divide(%r, %r, scale=%d)" % (self.children[0], self.children[1], self.scale)
        if self.op == EXPR_NULL:
            return "None"
        if self.op in (EXPR_IF, EXPR_COALESCE, EXPR_ABS, EXPR_IS_NULL):
            name = {EXPR_IF: "when", EXPR_COALESCE: "coalesce", EXPR_ABS: "abs", EXPR_IS_NULL: "is_null"}[self.op]
            return "%s(%s)" % (name, ", ".join(repr(c) for c in self.children))
        if self.op == EXPR_CAST:
            target = {PV_INT64: "'int64'", PV_FLOAT64: "'float64'"}.get(self.value_type) or "decimal(%d)" % self.scale
            return "cast(%r, %s)" % (self.children[0], target)
        if self.op == EXPR_ROUND:
            return "round_(%r, %d)" % (self.children[0], self.scale)
        if self.op in (EXPR_FLOOR, EXPR_CEIL, EXPR_TRUNC):
            return "%s(%r)" % ({EXPR_FLOOR: "floor", EXPR_CEIL: "ceil", EXPR_TRUNC: "trunc"}[self.op], self.children[0])
        if self.op == EXPR_NOT:
            return "(~%r)" % (self.children[0],)
        if self.op == EXPR_CMP:
            return "(%r %s %r)" % (self.children[0], _CMP_SIGNS[self.cmp], self.children[1])
        if self.op in (EXPR_AND, EXPR_OR):
            return "(%r %s %r)" % (self.children[0], "&" if self.op == EXPR_AND else "|", self.children[1])
        signs = {EXPR_ADD: "+", EXPR_SUB: "-", EXPR_MUL: "*", EXPR_DIV: "/", EXPR_FLOOR_DIV: "//", EXPR_MOD: "%"}
        return "(%r %s %r)" % (self.children[0], signs[self.op], self.children[1])

    def node_count(self):
        return 1 + sum(c.node_count() for c in self.children)

    def flatten(self):
        """-> (ctypes array of AggExprNode in pre-order, objects to keep alive): what Predicate.flatten does for a predicate."""
        out, keep = [], []

        def walk(e):
            n = AggExprNode()
            n.op = e.op
            if e.op == EXPR_COLUMN:
                keep.append(e.column.encode())
                n.column = keep[-1]
            elif e.op == EXPR_LITERAL:
                n.value_type = e.value_type
                if e.value_type == PV_DECIMAL128:
                    unscaled, scale = e.value
                    keep.append(int(unscaled).to_bytes(16, "little", signed=True))
                    n.s, n.s_len, n.i = keep[-1], 16, int(scale)
                elif e.value_type == PV_FLOAT64:
                    n.f = e.value
                else:
                    n.i = e.value
            elif e.op == EXPR_DATE_PART:
                n.i = e.part
            elif e.op == EXPR_DIV:
                n.i = -1 if e.scale is None else e.scale
            elif e.op == EXPR_CMP:
                n.i = e.cmp
            elif e.op == EXPR_CAST:
                n.value_type = e.value_type
                n.i = e.scale if e.value_type == PV_DECIMAL128 else 0
            elif e.op == EXPR_ROUND:
                n.i = e.scale
            out.append(n)
            for c in e.children:
                walk(c)

        walk(self)
        return (AggExprNode * len(out))(*out), keep


_WIDE = decimal.Context(prec=80)


def col(name):
    """A projected root column as an expression."""
    return Expr(EXPR_COLUMN, column=_column("col", name))


def lit(v):
    """A literal as an expression: an int (int64), a decimal.Decimal (a Decimal128 literal: at most 38 digits, scale 0 .. 38; a
    positive exponent is written out at scale 0) or a float.  bool is a TypeError; a NaN / Infinity Decimal, a magnitude of 10^38 or
    more unscaled, a scale past 38 and an int outside int64 are a ValueError."""
    if isinstance(v, bool) or not isinstance(v, (int, float, decimal.Decimal)):
        raise TypeError("lit: an int, a decimal.Decimal or a float, not %s" % type(v).__name__)
    if isinstance(v, int):
        if not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("lit: the int %d is outside int64" % v)
        return Expr(EXPR_LITERAL, value_type=PV_INT64, value=v)
    if isinstance(v, float):
        return Expr(EXPR_LITERAL, value_type=PV_FLOAT64, value=v)
    if not v.is_finite():
        raise ValueError("lit: the Decimal %r is not a finite number" % (v,))
    sign, digits, exponent = v.as_tuple()
    unscaled = int("".join(map(str, digits)) or "0")
    if exponent > 0:
        if unscaled and len(digits) + exponent > 38:
            raise ValueError("lit: the Decimal %r has a magnitude of 10^38 or more" % (v,))
        unscaled, exponent = unscaled * 10 ** exponent, 0
    if sign:
        unscaled = -unscaled
    if -exponent > 38 or abs(unscaled) >= 10 ** 38:
        raise ValueError("lit: the Decimal %r needs a scale of 0 .. 38 and an unscaled magnitude below 10^38" % (v,))
    return Expr(EXPR_LITERAL, value_type=PV_DECIMAL128, value=(unscaled, -exponent))


def divide(a, b, scale=None):
    """a / b (ORCGPU_AGG_EXPR_DIV) with the scale of an exact quotient chosen: a and b are an Expr, a column name or a number.
    Over integer and Decimal operands the result is a Decimal at `scale` (0 .. 38), the exact quotient rounded half away from zero;
    scale=None is what `a / b` gives: min(38, max(6, sa + 4)) for a dividend of scale sa.  Over doubles it is one IEEE division and
    the scale is not read.  A zero divisor, and a dividend that leaves 128 bits once it is taken times the power of ten the scale
    asks for, overflow the row."""
    if scale is not None:
        if isinstance(scale, bool) or not isinstance(scale, int):
            raise TypeError("divide: the scale is an int 0 .. 38 or None, not %s" % type(scale).__name__)
        if not 0 <= scale <= 38:
            raise ValueError("divide: the scale is 0 .. 38, got %d" % scale)
    ops = []
    for x in (a, b):
        if isinstance(x, str):
            x = col(x)
        elif not isinstance(x, Expr):
            if isinstance(x, bool) or not isinstance(x, (int, float, decimal.Decimal)):
                raise TypeError("divide: an Expr, a column name or a number, not %s" % type(x).__name__)
            x = lit(x)
        ops.append(x)
    return Expr(EXPR_DIV, ops, scale=scale)


def _operand(what, x, null_ok=False):
    """An operand of when / case / coalesce / nullif / abs_: an Expr that is a number, a column name, a number, or -- null_ok -- None."""
    if x is None and null_ok:
        return Expr(EXPR_NULL)
    if isinstance(x, str):
        return col(x)
    if isinstance(x, Expr):
        if x.op in _CONDITIONS:
            raise TypeError("%s: %r is a condition, not a number" % (what, x))
        return x
    if isinstance(x, bool) or not isinstance(x, (int, float, decimal.Decimal)):
        raise TypeError("%s: an Expr, a column name%s or a number, not %s" % (what, ", None" if null_ok else "", type(x).__name__))
    return lit(x)


def _condition(what, p):
    """A Predicate as the condition nodes of an expression (ORCGPU_AGG_EXPR_CMP / _IS_NULL / _AND / _OR / _NOT).  What has no such
    node -- LIKE, IN, in_set, a comparison with a string, Boolean, Timestamp or NULL value -- is a TypeError naming the leaf."""
    from . import predicate as P
    if not isinstance(p, Predicate):
        raise TypeError("%s: the condition is a Predicate (col('a') < 5, Predicate.is_null('a'), ...), not %s" % (what, type(p).__name__))
    if p.op == P.CMP_EXPR:
        return Expr(EXPR_CMP, p.exprs, cmp=p.cmp)
    if p.op in (P.IS_NULL, P.IS_NOT_NULL):
        e = Expr(EXPR_IS_NULL, (col(p.column),))
        return e if p.op == P.IS_NULL else Expr(EXPR_NOT, (e,))
    if p.op == P.NOT:
        if len(p.children) != 1:
            raise ValueError("%s: %r has not one operand" % (what, p))
        return Expr(EXPR_NOT, (_condition(what, p.children[0]),))
    if p.op in (P.AND, P.OR):
        if not p.children:
            raise ValueError("%s: %r has no operand" % (what, p))
        e = _condition(what, p.children[0])
        for c in p.children[1:]:
            e = Expr(EXPR_AND if p.op == P.AND else EXPR_OR, (e, _condition(what, c)))
        return e
    v = p.value
    if P.EQ <= p.op <= P.GE and isinstance(v, P.PredicateValue) and v.value is not None and not isinstance(v.value, bool):
        x = None
        if v.kind in (P.PV_INT8, P.PV_INT16, P.PV_INT32, P.PV_INT64):
            x = lit(int(v.value))
        elif v.kind in (P.PV_FLOAT32, P.PV_FLOAT64):
            x = lit(float(v.value))
        elif v.kind == P.PV_DECIMAL128:
            x = Expr(EXPR_LITERAL, value_type=PV_DECIMAL128, value=tuple(v.value))
        if x is not None:
            return Expr(EXPR_CMP, (col(p.column), x), cmp=p.op)
    raise TypeError("%s: the leaf %r cannot stand in an expression's condition -- only comparisons of numbers, is_null / is_not_null and "
                    "and_ / or_ / not_ over them can; condition an aggregate on it with Agg.where" % (what, p))


def when(cond, then, otherwise=None):
    """CASE WHEN cond THEN then ELSE otherwise END (ORCGPU_AGG_EXPR_IF): `then` where cond is TRUE, `otherwise` where it is FALSE
    or UNKNOWN.  cond: a Predicate -- what `col('a') < 5`, Expr.eq / ne and Predicate.compare return, Predicate.is_null /
    is_not_null, a plain numeric Predicate.comparison, and and_ / or_ / not_ over these.  then / otherwise: an Expr, a column name,
    a number, or None for NULL (not both).  The branch that is not taken may be NULL, divide by zero or overflow: nothing is seen
    of it.  Nest for more branches, or use case()."""
    c = _condition("when", cond)
    if then is None and otherwise is None:
        raise ValueError("when: both branches are None")
    return Expr(EXPR_IF, (c, _operand("when", then, True), _operand("when", otherwise, True)))


def case(branches, otherwise=None):
    """CASE WHEN c1 THEN a WHEN c2 THEN b ... ELSE otherwise END: branches is a non-empty list of (condition, value) pairs, nested
    into when() from the right."""
    if not isinstance(branches, (list, tuple)) or not branches:
        raise ValueError("case: a non-empty list of (condition, value) pairs")
    for b in branches:
        if not isinstance(b, (list, tuple)) or len(b) != 2:
            raise TypeError("case: every branch is a (condition, value) pair, not %r" % (b,))
    e = otherwise
    for cond, value in reversed(branches):
        e = when(cond, value, e)
    return e


def coalesce(a, b, *more):
    """COALESCE(a, b, ...) (ORCGPU_AGG_EXPR_COALESCE): the first operand that is not NULL; nested to the right."""
    xs = [_operand("coalesce", x) for x in (a, b) + more]
    e = xs[-1]
    for x in reversed(xs[:-1]):
        e = Expr(EXPR_COALESCE, (x, e))
    return e


def nullif(a, b):
    """NULLIF(a, b): NULL where a = b, else a -- `x / nullif(y, 0)`.  It is when(a.eq(b), None, a), with no node of its own: a's
    nodes are counted twice against the 32 of an expression."""
    a = _operand("nullif", a)
    return when(a.eq(_operand("nullif", b)), None, a)


def abs_(e):
    """|e| (ORCGPU_AGG_EXPR_ABS), also abs(expr): -2^127 overflows the row; a double has its sign bit cleared."""
    return Expr(EXPR_ABS, (_operand("abs_", e),))


class DecimalTarget:
    """decimal(scale): the Decimal128(38, scale) target of a cast."""

    def __init__(self, scale):
        if isinstance(scale, bool) or not isinstance(scale, int):
            raise TypeError("decimal: the scale is an int 0 .. 38, not %s" % type(scale).__name__)
        if not 0 <= scale <= 38:
            raise ValueError("decimal: the scale is 0 .. 38, got %d" % scale)
        self.scale = scale

    def __repr__(self):
        return "decimal(%d)" % self.scale


def decimal_(scale):
    """The target of cast(e, decimal_(scale)): Decimal128(38, scale), scale 0 .. 38.  `decimal_` here -- `decimal` is the standard
    library's module in this one --; the package also exports it under the name `orc_rust_amd.decimal`."""
    return DecimalTarget(scale)


def cast(e, target):
    """CAST(e AS target) (ORCGPU_AGG_EXPR_CAST).  e: an Expr, a column name or a number; target: "int64", "float64" or
    decimal_(scale) (orc_rust_amd.decimal(scale): the same function).  To float64: the double nearest the exact value (of a Decimal: unscaled / 10^scale), ties to even.  To
    decimal(t): an integer or a Decimal of a lower scale times the power of ten; a Decimal of a higher scale divided by it, half away
    from zero; a double's exact value times 10^t, half away from zero.  To int64: truncated toward zero.  NaN, an infinity and a value
    the target cannot hold overflow the row."""
    x = _operand("cast", e)
    if isinstance(target, DecimalTarget):
        return Expr(EXPR_CAST, (x,), value_type=PV_DECIMAL128, scale=target.scale)
    if not isinstance(target, str):
        raise TypeError("cast: the target is 'int64', 'float64' or decimal(scale), not %s" % type(target).__name__)
    if target not in ("int64", "float64"):
        raise ValueError("cast: the target is 'int64', 'float64' or decimal(scale), got %r" % target)
    return Expr(EXPR_CAST, (x,), value_type=PV_INT64 if target == "int64" else PV_FLOAT64)


def round_(e, digits=0):
    """ROUND(e, digits) (ORCGPU_AGG_EXPR_ROUND), also round(expr, digits): a Decimal of a higher scale is brought to `digits`
    places (0 .. 38), half away from zero; an integer is unchanged; a double takes digits = 0 alone -- C's round(), still a double:
    round a double to n places with cast(e, decimal_(n))."""
    x = _operand("round_", e)
    if isinstance(digits, bool) or not isinstance(digits, int):
        raise TypeError("round_: the digits are an int 0 .. 38, not %s" % type(digits).__name__)
    if not 0 <= digits <= 38:
        raise ValueError("round_: the digits are 0 .. 38, got %d" % digits)
    return Expr(EXPR_ROUND, (x,), scale=digits)


def floor(e):
    """FLOOR(e) (ORCGPU_AGG_EXPR_FLOOR), also math.floor(expr): a Decimal -> the integer at scale 0 toward -infinity; an integer
    unchanged; a double -> IEEE floor, still a double."""
    return Expr(EXPR_FLOOR, (_operand("floor", e),))


def ceil(e):
    """CEIL(e) (ORCGPU_AGG_EXPR_CEIL), also math.ceil(expr): toward +infinity."""
    return Expr(EXPR_CEIL, (_operand("ceil", e),))


def trunc(e):
    """TRUNC(e) (ORCGPU_AGG_EXPR_TRUNC), also math.trunc(expr): toward zero."""
    return Expr(EXPR_TRUNC, (_operand("trunc", e),))


def extract(part, e):
    """SQL's extract(part from e) (ORCGPU_AGG_EXPR_DATE_PART): a calendar field of a Date.  part: one of DATE_PARTS -- "year",
    "quarter" (1 .. 4), "month" (1 .. 12), "day" (1 .. 31), "day_of_week" (ISO: Monday = 1 .. Sunday = 7), "day_of_year" (1 .. 366).
    e: a column name, or an Expr over Byte / Short / Int / Long / Date columns and ints whose value is a number of days since
    1970-01-01 (`col("d") + 30`).  Proleptic Gregorian, year 0 exists.  The result is an integer; days outside int32 overflow the
    row.  year(e), quarter(e), month(e), day(e), day_of_week(e) and day_of_year(e) are extract with the part named."""
    if not isinstance(part, str):
        raise TypeError("extract: the part is a str (one of %s), not %s" % (", ".join(DATE_PARTS), type(part).__name__))
    if part not in DATE_PARTS:
        raise ValueError("extract: the part is one of %s, got %r" % (", ".join(DATE_PARTS), part))
    if isinstance(e, str):
        e = col(e)
    if not isinstance(e, Expr):
        raise TypeError("%s: an Expr or a column name, not %s" % (part, type(e).__name__))
    return Expr(EXPR_DATE_PART, (e,), part=DATE_PARTS.index(part))


def year(e):
    return extract("year", e)


def quarter(e):
    return extract("quarter", e)


def month(e):
    return extract("month", e)


def day(e):
    return extract("day", e)


def day_of_week(e):
    return extract("day_of_week", e)


def day_of_year(e):
    return extract("day_of_year", e)


class Agg:
    """One aggregate: Agg.count_rows(), .count(c), .sum(c), .avg(c), .min(c), .max(c), .sum_product(a, b); sum and avg take a column
    name or an Expr.  .where(predicate) conditions any of them: agg(x) FILTER (WHERE predicate)."""

    def __init__(self, op, column=None, column2=None, expr=None, filter=None):
        self.op, self.column, self.column2, self.expr, self.filter = op, column, column2, expr, filter

    def where(self, predicate):
        """A new Agg over the kept rows for which `predicate` (a orc_rust_amd.predicate.Predicate over projected root columns, in
        the row filter's language) is TRUE: SQL's agg(x) FILTER (WHERE predicate), i.e. agg(CASE WHEN predicate THEN x END).  One
        condition an aggregate: combine several with Predicate.and_ first."""
        if not isinstance(predicate, Predicate):
            raise TypeError("Agg.where: a Predicate, not %s" % type(predicate).__name__)
        if self.filter is not None:
            raise ValueError("Agg.where: %r has a condition already; combine the two with Predicate.and_([...])" % (self,))
        return Agg(self.op, self.column, self.column2, self.expr, predicate)

    @classmethod
    def count_rows(cls):
        return cls(COUNT_ROWS)

    @classmethod
    def count(cls, column):
        return cls(COUNT, _column("Agg.count", column))

    @classmethod
    def sum(cls, column):
        if isinstance(column, Expr):
            return cls(SUM_EXPR, expr=column)
        return cls(SUM, _column("Agg.sum", column))

    @classmethod
    def avg(cls, column):
        if isinstance(column, Expr):
            return cls(AVG_EXPR, expr=column)
        return cls(AVG, _column("Agg.avg", column))

    @classmethod
    def min(cls, column):
        return cls(MIN, _column("Agg.min", column))

    @classmethod
    def max(cls, column):
        return cls(MAX, _column("Agg.max", column))

    @classmethod
    def sum_product(cls, column, column2):
        return cls(SUM_PRODUCT, _column("Agg.sum_product", column), _column("Agg.sum_product", column2))

    def __repr__(self):
        text = "Agg.%s(%s)" % (_NAMES[self.op], ", ".join(repr(c) for c in (self.column, self.column2, self.expr) if c is not None))
        return text if self.filter is None else "%s.where(%r)" % (text, self.filter)


class TimestampValue(int):
    """MIN / MAX of a Timestamp column: the int64 in the unit the column is decoded to, with `.units` ('s', 'ms', 'us', 'ns')."""
    units = "ns"


def check_specs(specs):
    """The argument of aggregate(), checked before anything reaches the GPU: a non-empty list or tuple of at most 64 Agg."""
    if not isinstance(specs, (list, tuple)):
        raise TypeError("aggregate: a list or tuple of Agg, not %s" % type(specs).__name__)
    for s in specs:
        if not isinstance(s, Agg):
            raise TypeError("aggregate: every spec is an Agg (Agg.sum('column'), ...), not %s" % type(s).__name__)
    if not specs:
        raise ValueError("aggregate: an empty list of aggregates")
    if len(specs) > AGG_MAX:
        raise ValueError("aggregate: %d aggregates, at most %d in one list" % (len(specs), AGG_MAX))
    return list(specs)


def check_group_by(group_by):
    """The group_by argument of aggregate(), checked before anything reaches the GPU: a list or tuple of 1 .. 4 distinct non-empty
    str.  Returns it as a list."""
    if not isinstance(group_by, (list, tuple)):
        raise TypeError("aggregate: group_by is a list or tuple of column names, not %s" % type(group_by).__name__)
    seen = set()
    for name in group_by:
        _column("aggregate: group_by", name)
        if name in seen:
            raise ValueError("aggregate: group_by lists column %r twice" % name)
        seen.add(name)
    if not group_by:
        raise ValueError("aggregate: an empty group_by")
    if len(group_by) > GROUP_MAX_KEYS:
        raise ValueError("aggregate: %d group_by columns, at most %d" % (len(group_by), GROUP_MAX_KEYS))
    return list(group_by)


def check_group_limits(max_groups, max_total_groups, group_by):
    """The max_groups / max_total_groups arguments of aggregate(), checked before anything reaches the GPU: each None (the
    default: 256 / 65536) or an int -- not a bool -- of 1 .. 2^20 / 1 .. 2^24, the total not below the limit of one stripe, and
    neither without a group_by.  Returns them as the C calls take them: 0 for None."""
    for what, v, top in (("max_groups", max_groups, GROUP_LIMIT_MAX), ("max_total_groups", max_total_groups, GROUP_TOTAL_LIMIT_MAX)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("aggregate: %s is an int, not %s (%r)" % (what, type(v).__name__, v))
        if not 1 <= v <= top:
            raise ValueError("aggregate: %s is %d, not in 1 .. %d" % (what, v, top))
        if group_by is None:
            raise ValueError("aggregate: %s = %d without a group_by" % (what, v))
    groups = GROUP_MAX if max_groups is None else max_groups
    total = GROUP_MAX_TOTAL if max_total_groups is None else max_total_groups
    if total < groups:
        raise ValueError("aggregate: max_total_groups is %d, below max_groups = %d" % (total, groups))
    return max_groups or 0, max_total_groups or 0


def key_array(group_by):
    """[str] -> ctypes array of char*"""
    names = check_group_by(group_by)
    return (C.c_char_p * len(names))(*[n.encode() for n in names])


def spec_array(specs):
    """[Agg] -> (ctypes array of orcgpu_agg_spec, what keeps its strings alive)"""
    specs = check_specs(specs)
    arr = (AggSpec * len(specs))()
    keep = []
    for i, s in enumerate(specs):
        arr[i].op = s.op
        for field, name in (("column", s.column), ("column2", s.column2)):
            if name is not None:
                keep.append(name.encode())
                setattr(arr[i], field, keep[-1])
    return arr, keep


def expr_array(specs):
    """[Agg] -> (ctypes array of orcgpu_agg_expr parallel to spec_array's, what keeps its nodes alive), or (None, []) when no
    spec holds an Expr: the bindings then call the entry points without expressions."""
    specs = check_specs(specs)
    if not any(s.expr is not None for s in specs):
        return None, []
    arr = (AggExpr * len(specs))()
    keep = []
    for i, s in enumerate(specs):
        if s.expr is None:
            continue
        nodes, alive = s.expr.flatten()
        keep.append((nodes, alive))
        arr[i].nodes = nodes
        arr[i].n_nodes = len(nodes)
    return arr, keep


def filter_array(specs):
    """[Agg] -> (ctypes array of orcgpu_agg_filter parallel to spec_array's, what keeps its nodes alive), or (None, []) when no
    spec has a condition: the bindings then call the entry points without conditions."""
    specs = check_specs(specs)
    if not any(s.filter is not None for s in specs):
        return None, []
    arr = (AggFilter * len(specs))()
    keep = []
    for i, s in enumerate(specs):
        if s.filter is None:
            continue
        nodes, alive = s.filter.flatten()
        keep.append((nodes, alive))
        arr[i].nodes = nodes
        arr[i].n_nodes = len(nodes)
    return arr, keep


def _signed(words, bits):
    v = sum(int(w) << (64 * k) for k, w in enumerate(words))
    return v - (1 << bits) if v >> (bits - 1) else v


def value_of(v, spec):
    """orcgpu_agg_value -> int / decimal.Decimal / float / None; OverflowError, naming the spec, when its overflow flag is set."""
    if v.overflow:
        raise OverflowError("aggregate: %r left the range of its result" % (spec,))
    if v.is_null:
        return None
    if v.kind == KIND_U64:
        return int(v.w[0])
    if v.kind == KIND_I128:
        return _signed(v.w[:2], 128)
    if v.kind == KIND_DEC128:
        with decimal.localcontext() as c:
            c.prec = 60
            return decimal.Decimal(_signed(v.w[:2], 128)).scaleb(-v.scale_or_unit)
    if v.kind == KIND_F64:
        return float(v.f)
    x = _signed(v.w[:1], 64)
    if 0 <= v.scale_or_unit < len(TS_UNITS):  # (a Timestamp column: -1 for every other int64 result)
        x = TimestampValue(x)
        x.units = TS_UNITS[v.scale_or_unit]
    return x


def values_of(arr, specs):
    return [value_of(v, s) for v, s in zip(arr, specs)]


def key_of(k):
    """orcgpu_group_key -> int / bool / decimal.Decimal / TimestampValue / str / None; a String key whose bytes are not valid
    UTF-8 comes back as bytes."""
    if k.is_null:
        return None
    if k.kind == GROUP_KEY_BOOL:
        return bool(k.w[0])
    if k.kind == GROUP_KEY_DEC128:
        with decimal.localcontext() as c:
            c.prec = 60
            return decimal.Decimal(_signed(k.w[:2], 128)).scaleb(-k.scale_or_unit)
    if k.kind == GROUP_KEY_STRING:
        raw = bytes(k.bytes[:min(k.len, GROUP_KEY_BYTES)])
        try:
            return raw.decode("utf-8")
        except UnicodeDecodeError:
            return raw
    x = _signed(k.w[:1], 64)
    if 0 <= k.scale_or_unit < len(TS_UNITS):
        x = TimestampValue(x)
        x.units = TS_UNITS[k.scale_or_unit]
    return x


def groups_of(L, handle, n_keys, specs, raw=False):
    """An orcgpu_groups handle -> [(keys tuple, values list)] in first-appearance order; the handle is freed.  raw=True: the values
    are the orcgpu_agg_value records.  OverflowError names the spec and the group's keys."""
    try:
        out = []
        for g in range(L.orcgpu_groups_count(handle)):
            keys = []
            for k in range(n_keys):
                rec = GroupKey()
                if L.orcgpu_groups_key(handle, g, k, C.byref(rec)):
                    raise RuntimeError("orcgpu_groups_key(%d, %d)" % (g, k))
                keys.append(key_of(rec))
            vals = []
            for i, s in enumerate(specs):
                v = AggValue()
                if L.orcgpu_groups_value(handle, g, i, C.byref(v)):
                    raise RuntimeError("orcgpu_groups_value(%d, %d)" % (g, i))
                if raw:
                    vals.append(v)
                    continue
                try:
                    vals.append(value_of(v, s))
                except OverflowError:
                    raise OverflowError("aggregate: %r left the range of its result in the group %r" % (s, tuple(keys))) from None
            out.append((tuple(keys), vals))
        return out
    finally:
        L.orcgpu_groups_free(handle)
