"""Host-side mirror of the reference's predicate API (src/predicate.rs): `Predicate` / `PredicateValue` / `ComparisonOp`,
flattened to the pre-order node list of include/orcgpu.h (orcgpu_predicate_node) for orcgpu_reader_set_predicate and
orcgpu_predicate_row_groups."""
import ctypes as C
import datetime
import decimal

EQ, NE, LT, LE, GT, GE, IS_NULL, IS_NOT_NULL, AND, OR, NOT = range(11)
LIKE = 16  # (11 .. 15 are unknown ops)
IN, LITERAL = 17, 18  # an IN leaf, and one value of its list
IN_SET = 26  # x IN SET s: a leaf whose i names a sealed key_set.KeySet
CMP_EXPR = 19  # lhs OP rhs over two arithmetic expressions; its subtrees are made of the nodes below
EXPR_COLUMN, EXPR_LITERAL, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG = range(20, 26)  # ORCGPU_PRED_EXPR_*: aggregate.EXPR_* + 20
EXPR_DATE_PART = 36  # ... aggregate.EXPR_DATE_PART + 20: one child, the part in `i`
EXPR_DIV, EXPR_FLOOR_DIV, EXPR_MOD = 37, 38, 39  # ... aggregate.EXPR_DIV .. EXPR_MOD + 20: two children; DIV: the result scale, or -1, in `i`
# ... aggregate.EXPR_IF .. EXPR_NOT + 20: the conditionals (3, 2, 1, 0, 2, 1, 2, 2, 1 children; CMP: the comparison EQ .. GE in `i`)
EXPR_IF, EXPR_COALESCE, EXPR_ABS, EXPR_NULL, EXPR_CMP, EXPR_IS_NULL, EXPR_AND, EXPR_OR, EXPR_NOT = range(41, 50)
# ... aggregate.EXPR_CAST .. EXPR_TRUNC + 20: the conversions, one child each (CAST: the target in value_type, a Decimal's scale in `i`;
# ROUND: the digits in `i`)
EXPR_CAST, EXPR_ROUND, EXPR_FLOOR, EXPR_CEIL, EXPR_TRUNC = range(50, 55)
_CMP_OPS = {"=": EQ, "!=": NE, "<": LT, "<=": LE, ">": GT, ">=": GE}
_CMP_SIGNS = {v: k for k, v in _CMP_OPS.items()}
PV_BOOLEAN, PV_INT8, PV_INT16, PV_INT32, PV_INT64, PV_FLOAT32, PV_FLOAT64, PV_UTF8, PV_DECIMAL128, PV_TIMESTAMP_NS = range(10)
_EPOCH = datetime.datetime(1970, 1, 1)


_PV_NAMES = ("Boolean", "Int8", "Int16", "Int32", "Int64", "Float32", "Float64", "Utf8", "Decimal128", "TimestampNs")
_OP_NAMES = {EQ: "eq", NE: "ne", LT: "lt", LE: "lte", GT: "gt", GE: "gte", IS_NULL: "is_null", IS_NOT_NULL: "is_not_null", AND: "and_", OR: "or_", NOT: "not_",
             LIKE: "like", IN: "in_list", IN_SET: "in_set"}


class PredicateNode(C.Structure):
    _fields_ = [("op", C.c_int32), ("n_children", C.c_uint32), ("column", C.c_char_p), ("value_type", C.c_int32), ("value_is_null", C.c_int32),
                ("i", C.c_int64), ("f", C.c_double), ("s", C.c_char_p), ("s_len", C.c_uint64)]


class ColumnIndex(C.Structure):
    _fields_ = [("name", C.c_char_p), ("row_index", C.c_void_p), ("row_index_len", C.c_uint64), ("bloom_index", C.c_void_p),
                ("bloom_index_len", C.c_uint64)]


class PredicateValue:
    """PredicateValue::{Boolean, Int8, ..., Utf8}(Option<_>) (predicate.rs:29-47): value None = the SQL NULL literal.
    Decimal128 and TimestampNs are this library's own (include/orcgpu.h: ORCGPU_PV_DECIMAL128, ORCGPU_PV_TIMESTAMP_NS); their
    .value is the (unscaled, scale) pair and the nanoseconds since 1970-01-01T00:00:00."""

    def __init__(self, kind, value):
        self.kind, self.value = kind, value

    def __repr__(self):
        return "%s(%r)" % (_PV_NAMES[self.kind], self.value)

    Boolean = classmethod(lambda cls, v: cls(PV_BOOLEAN, v))
    Int8 = classmethod(lambda cls, v: cls(PV_INT8, v))
    Int16 = classmethod(lambda cls, v: cls(PV_INT16, v))
    Int32 = classmethod(lambda cls, v: cls(PV_INT32, v))
    Int64 = classmethod(lambda cls, v: cls(PV_INT64, v))
    Float32 = classmethod(lambda cls, v: cls(PV_FLOAT32, v))
    Float64 = classmethod(lambda cls, v: cls(PV_FLOAT64, v))
    Utf8 = classmethod(lambda cls, v: cls(PV_UTF8, v))

    @classmethod
    def Decimal128(cls, v):
        """v: a decimal.Decimal, an (unscaled, scale) pair with scale 0 .. 38 and |unscaled| < 10^38, or None."""
        if v is None:
            return cls(PV_DECIMAL128, None)
        if isinstance(v, decimal.Decimal):
            if not v.is_finite():
                raise ValueError("Decimal128 literal: %r is not a finite number" % (v,))
            sign, digits, exponent = v.as_tuple()
            if exponent > 0:
                raise ValueError("Decimal128 literal: %r has a positive exponent; quantize it to the scale that is meant" % (v,))
            unscaled, scale = int("".join(map(str, digits)) or "0"), -exponent
            if sign:
                unscaled = -unscaled
        else:
            unscaled, scale = v
            if isinstance(unscaled, bool) or isinstance(scale, bool) or not isinstance(unscaled, int) or not isinstance(scale, int):
                raise TypeError("Decimal128 literal: (unscaled, scale) are integers, got %r" % (v,))
        if not 0 <= scale <= 38 or abs(unscaled) >= 10 ** 38:
            raise ValueError("Decimal128 literal: scale %d, unscaled %d: the scale is 0 .. 38 and the magnitude below 10^38" % (scale, unscaled))
        return cls(PV_DECIMAL128, (unscaled, scale))

    @classmethod
    def TimestampNs(cls, v):
        """v: integer nanoseconds since 1970-01-01T00:00:00, a datetime.datetime (naive: read as wall clock; aware: converted to
        UTC) or None.  In the sense of the column's exported value: wall clock for TIMESTAMP, UTC for TIMESTAMP_INSTANT."""
        if v is None:
            return cls(PV_TIMESTAMP_NS, None)
        if isinstance(v, datetime.datetime):
            if v.tzinfo is not None and v.utcoffset() is not None:
                v = (v - v.utcoffset()).replace(tzinfo=None)
            else:
                v = v.replace(tzinfo=None)
            d = v - _EPOCH  # (days, seconds, microseconds): exact integers, no float on the way
            v = ((d.days * 86400 + d.seconds) * 10 ** 6 + d.microseconds) * 1000
        elif isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("TimestampNs literal: an int or a datetime.datetime, got %r" % (v,))
        if not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("TimestampNs literal: %d ns is outside int64 (1677-09-21 .. 2262-04-11)" % v)
        return cls(PV_TIMESTAMP_NS, v)


class Predicate:
    """Predicate::{Comparison, IsNull, IsNotNull, And, Or, Not} with the reference's constructors (predicate.rs:98-180), and
    this library's own LIKE leaf (like / not_like / starts_with / ends_with / contains), IN leaf (in_list / not_in) and
    expression leaf (compare: lhs OP rhs over arithmetic expressions of columns and literals)."""

    def __init__(self, op, column=None, value=None, children=()):
        self.op, self.column, self.value, self.children = op, column, value, list(children)
        self.escape = None  # LIKE: the escape character
        self.cmp, self.exprs = None, ()  # CMP_EXPR: EQ .. GE, and the two sides (aggregate.Expr)

    @classmethod
    def compare(cls, lhs, op, rhs):
        """lhs OP rhs (ORCGPU_PRED_CMP_EXPR, this library's own): each side an aggregate.Expr -- col(name), lit(v), + - * and
        unary - -- or a plain int / float / decimal.Decimal, which lit() wraps; op one of "=", "!=", "<", "<=", ">", ">=".
        Evaluated exactly, per row, on the GPU: UNKNOWN where a column of either side is NULL or an operation inside a side leaves
        128 bits.  `col("a") < col("b")`, `.eq(x)` and `.ne(x)` on an Expr build the same."""
        from .aggregate import Expr, lit  # (aggregate.py imports this module)
        if not isinstance(op, str) or op not in _CMP_OPS:
            raise ValueError("Predicate.compare: the operator is one of %s, got %r" % (", ".join(sorted(_CMP_OPS)), op))
        sides = []
        for x in (lhs, rhs):
            if not isinstance(x, Expr):
                try:
                    x = lit(x)
                except TypeError:
                    raise TypeError("Predicate.compare: a side is an Expr, an int, a float or a decimal.Decimal, not %s" % type(x).__name__) from None
            sides.append(x)
        p = cls(CMP_EXPR)
        p.cmp, p.exprs = _CMP_OPS[op], tuple(sides)
        return p

    @classmethod
    def comparison(cls, column, op, value):
        return cls(op, column, value)

    eq = classmethod(lambda cls, c, v: cls(EQ, c, v))
    ne = classmethod(lambda cls, c, v: cls(NE, c, v))
    lt = classmethod(lambda cls, c, v: cls(LT, c, v))
    lte = classmethod(lambda cls, c, v: cls(LE, c, v))
    gt = classmethod(lambda cls, c, v: cls(GT, c, v))
    gte = classmethod(lambda cls, c, v: cls(GE, c, v))
    is_null = classmethod(lambda cls, c: cls(IS_NULL, c))
    is_not_null = classmethod(lambda cls, c: cls(IS_NOT_NULL, c))

    @classmethod
    def like(cls, column, pattern, escape=None):
        """SQL LIKE on a String / Varchar / Char column (ORCGPU_PRED_LIKE, this library's own): `%` any run of bytes, `_` one code
        point, `escape` (one ASCII character, or None) makes the pattern character behind it a literal.  pattern: str (encoded to
        UTF-8), bytes, or None for the NULL pattern.  The whole value must match."""
        if escape is not None and not (isinstance(escape, str) and len(escape) == 1 and 0 < ord(escape) < 128):
            raise ValueError("LIKE escape: one ASCII character or None, got %r" % (escape,))
        if pattern is not None and not isinstance(pattern, (str, bytes, bytearray)):
            raise ValueError("LIKE pattern: a str, bytes or None, got %r" % (pattern,))
        p = cls(LIKE, column, PredicateValue(PV_UTF8, pattern))
        p.escape = escape
        return p

    @classmethod
    def not_like(cls, column, pattern, escape=None):
        return cls.not_(cls.like(column, pattern, escape))

    @staticmethod
    def _like_literal(text):
        """text with `%`, `_` and the escape character itself escaped by a backslash"""
        if isinstance(text, str):
            return text.replace("\\", "\\\\").replace("%", "\\%").replace("_", "\\_")
        return bytes(text).replace(b"\\", b"\\\\").replace(b"%", b"\\%").replace(b"_", b"\\_")

    @classmethod
    def starts_with(cls, column, text):
        lit = cls._like_literal(text)
        return cls.like(column, lit + ("%" if isinstance(lit, str) else b"%"), escape="\\")

    @classmethod
    def ends_with(cls, column, text):
        lit = cls._like_literal(text)
        return cls.like(column, ("%" if isinstance(lit, str) else b"%") + lit, escape="\\")

    @classmethod
    def contains(cls, column, text):
        lit = cls._like_literal(text)
        pc = "%" if isinstance(lit, str) else b"%"
        return cls.like(column, pc + lit + pc, escape="\\")

    @classmethod
    def in_list(cls, column, values):
        """SQL IN (ORCGPU_PRED_IN, this library's own): column IN (values), exactly the OR of column = v over the values under
        three-valued logic -- the empty list is FALSE, a NULL among the values makes every non-match UNKNOWN.  values: an iterable
        of PredicateValue of the kinds the column takes (at most 65536 of them)."""
        if isinstance(values, (PredicateValue, str, bytes)):
            raise TypeError("IN list: an iterable of PredicateValue, got %r" % (values,))
        try:
            values = list(values)
        except TypeError:
            raise TypeError("IN list: an iterable of PredicateValue, got %r" % (values,)) from None
        for v in values:
            if not isinstance(v, PredicateValue):
                raise TypeError("IN list: every value is a PredicateValue, got %r" % (v,))
        return cls(IN, column, children=[cls(LITERAL, value=v) for v in values])

    @classmethod
    def not_in(cls, column, values):
        return cls.not_(cls.in_list(column, values))

    @classmethod
    def in_set(cls, column, key_set):
        """A semi-join (ORCGPU_PRED_IN_SET, this library's own): column IN SET key_set, where key_set is a sealed
        orc_rust_amd.KeySet -- the distinct keys an ArrowReaderBuilder.collect_keys left on the GPU.  Exactly in_list over the values
        the build side's kept rows held, NULLs included: a NULL row is UNKNOWN, the empty set FALSE, and a NULL on the build side
        makes every non-match UNKNOWN.  The column is a Byte, Short, Int, Long or Date column."""
        from .key_set import KeySet
        if not isinstance(column, str):
            raise TypeError("in_set: the column is a str, not %s" % type(column).__name__)
        if not isinstance(key_set, KeySet):
            raise TypeError("in_set: the set is a KeySet (ArrowReaderBuilder.collect_keys), not %s" % type(key_set).__name__)
        p = cls(IN_SET, column)
        p.key_set = key_set  # (kept alive with the predicate)
        return p

    @classmethod
    def not_in_set(cls, column, key_set):
        return cls.not_(cls.in_set(column, key_set))

    @classmethod
    def between(cls, column, lo, hi):
        """lo <= column <= hi: and_([gte(column, lo), lte(column, hi)])"""
        return cls.and_([cls.gte(column, lo), cls.lte(column, hi)])

    @classmethod
    def and_(cls, predicates):
        return cls(AND, children=predicates)

    @classmethod
    def or_(cls, predicates):
        return cls(OR, children=predicates)

    @classmethod
    def not_(cls, predicate):
        return cls(NOT, children=[predicate])

    # p & q, p | q, ~p: and_([p, q]), or_([p, q]), not_(p)
    def __and__(self, other):
        return Predicate.and_([self, other]) if isinstance(other, Predicate) else NotImplemented

    def __or__(self, other):
        return Predicate.or_([self, other]) if isinstance(other, Predicate) else NotImplemented

    def __invert__(self):
        return Predicate.not_(self)

    def __repr__(self):
        name = _OP_NAMES.get(self.op, "op%d" % self.op)
        if self.op in (AND, OR):
            return "%s(%r)" % (name, self.children)
        if self.op == NOT:
            return "not_(%r)" % (self.children[0],)
        if self.op in (IS_NULL, IS_NOT_NULL):
            return "%s(%r)" % (name, self.column)
        if self.op == IN:
            return "in_list(%r, %r)" % (self.column, [c.value for c in self.children])
        if self.op == IN_SET:
            return "in_set(%r, %r)" % (self.column, self.key_set)
        if self.op == CMP_EXPR:
            return "(%r %s %r)" % (self.exprs[0], _CMP_SIGNS[self.cmp], self.exprs[1])
        if self.op == LIKE:
            return "like(%r, %r%s)" % (self.column, self.value.value, "" if self.escape is None else ", escape=%r" % self.escape)
        return "%s(%r, %r)" % (name, self.column, self.value)

    def flatten(self):
        """-> (ctypes array of PredicateNode in pre-order, objects to keep alive)."""
        out, keep = [], []

        def walk_expr(e):  # aggregate.Expr -> ORCGPU_PRED_EXPR_* nodes, filled as Expr.flatten fills an AggExprNode
            n = PredicateNode()
            n.op = e.op + EXPR_COLUMN
            n.n_children = len(e.children)
            if e.op + EXPR_COLUMN == EXPR_COLUMN:
                keep.append(e.column.encode())
                n.column = keep[-1]
            elif e.op + EXPR_COLUMN == EXPR_LITERAL:
                n.value_type = e.value_type
                if e.value_type == PV_DECIMAL128:
                    unscaled, scale = e.value
                    keep.append(int(unscaled).to_bytes(16, "little", signed=True))
                    n.s, n.s_len, n.i = keep[-1], 16, int(scale)
                elif e.value_type == PV_FLOAT64:
                    n.f = e.value
                else:
                    n.i = e.value
            elif e.op + EXPR_COLUMN == EXPR_DATE_PART:
                n.i = e.part
            elif e.op + EXPR_COLUMN == EXPR_DIV:
                n.i = -1 if e.scale is None else e.scale
            elif e.op + EXPR_COLUMN == EXPR_CMP:
                n.i = e.cmp
            elif e.op + EXPR_COLUMN == EXPR_CAST:
                n.value_type = e.value_type
                n.i = e.scale if e.value_type == PV_DECIMAL128 else 0
            elif e.op + EXPR_COLUMN == EXPR_ROUND:
                n.i = e.scale
            out.append(n)
            for c in e.children:
                walk_expr(c)

        def walk(p):
            n = PredicateNode()
            n.op = p.op
            n.n_children = len(p.children)
            if p.op == CMP_EXPR:
                n.n_children, n.i = 2, p.cmp
                out.append(n)
                for e in p.exprs:
                    walk_expr(e)
                return
            if p.column is not None:
                b = p.column.encode()
                keep.append(b)
                n.column = b
            v = p.value
            if v is not None:
                n.value_type = v.kind
                n.value_is_null = 1 if v.value is None else 0
                if v.value is not None:
                    if v.kind == PV_UTF8:
                        b = v.value.encode() if isinstance(v.value, str) else bytes(v.value)
                        keep.append(b)
                        n.s, n.s_len = b, len(b)
                    elif v.kind == PV_DECIMAL128:
                        unscaled, scale = v.value
                        b = int(unscaled).to_bytes(16, "little", signed=True)
                        keep.append(b)
                        n.s, n.s_len, n.i = b, 16, int(scale)
                    elif v.kind in (PV_FLOAT32, PV_FLOAT64):
                        n.f = float(v.value)
                    else:
                        n.i = int(v.value)
            if p.op == LIKE:
                n.i = ord(p.escape) if p.escape else 0
            if p.op == IN_SET:
                n.i = p.key_set.id()
                keep.append(p.key_set)
            out.append(n)
            for c in p.children:
                walk(c)

        walk(self)
        arr = (PredicateNode * len(out))(*out)
        return arr, keep
