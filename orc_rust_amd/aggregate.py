"""Aggregates over the kept rows, reduced on the GPU (include/orcgpu.h: orcgpu_result_aggregate, orcgpu_reader_set_aggregates,
orcgpu_reader_aggregate): the specs a caller writes, their C form, and the Python values the results become.

    from orc_rust_amd.aggregate import Agg
    total, = ArrowReaderBuilder.try_new("lineitem.orc").with_projection([...]).with_row_filter(q6).aggregate(
        [Agg.sum_product("l_extendedprice", "l_discount")])          # a decimal.Decimal

Pure plumbing: nothing is computed here, and every argument is checked before anything reaches the GPU."""
import ctypes as C
import decimal

COUNT_ROWS, COUNT, SUM, MIN, MAX, SUM_PRODUCT = range(6)  # ORCGPU_AGG_OP_*
KIND_U64, KIND_I128, KIND_DEC128, KIND_F64, KIND_I64 = range(5)  # ORCGPU_AGG_KIND_*
AGG_MAX = 64  # ORCGPU_AGG_MAX
GROUP_KEY_I64, GROUP_KEY_DEC128, GROUP_KEY_BOOL, GROUP_KEY_STRING = range(4)  # ORCGPU_GROUP_KEY_*
GROUP_MAX_KEYS, GROUP_MAX, GROUP_MAX_TOTAL, GROUP_KEY_BYTES = 4, 256, 65536, 64  # ORCGPU_GROUP_*
_NAMES = ("count_rows", "count", "sum", "min", "max", "sum_product")
TS_UNITS = ("s", "ms", "us", "ns")


class AggSpec(C.Structure):
    _fields_ = [("op", C.c_uint32), ("column", C.c_char_p), ("column2", C.c_char_p)]


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


class Agg:
    """One aggregate: Agg.count_rows(), .count(c), .sum(c), .min(c), .max(c), .sum_product(a, b)."""

    def __init__(self, op, column=None, column2=None):
        self.op, self.column, self.column2 = op, column, column2

    @classmethod
    def count_rows(cls):
        return cls(COUNT_ROWS)

    @classmethod
    def count(cls, column):
        return cls(COUNT, _column("Agg.count", column))

    @classmethod
    def sum(cls, column):
        return cls(SUM, _column("Agg.sum", column))

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
        return "Agg.%s(%s)" % (_NAMES[self.op], ", ".join(repr(c) for c in (self.column, self.column2) if c is not None))


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
