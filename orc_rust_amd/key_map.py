"""KeyMap: the build side of a many-to-one equi-join (include/orcgpu.h: orcgpu_key_map) -- a KeySet that also holds, per distinct
non-NULL key of the kept rows of one or more reads, one row of 1 .. 8 value columns, in HBM beside the keys.  The keys must be
unique: a key that comes twice fails the seal ("duplicate key").

    om = ArrowReaderBuilder.try_new("orders.orc").collect_map("o_orderkey", ["o_orderdate", "o_shippriority"])     # sealed
    (ArrowReaderBuilder.try_new("lineitem.orc", ctx=om.ctx)
        .with_lookup_columns(om, "l_orderkey", {"o_orderdate": "o_orderdate", "o_shippriority": "o_shippriority"})
        .aggregate([Agg.sum("l_extendedprice")], group_by=["o_orderdate", "o_shippriority"]))

A lookup column is NULL where the probe key is NULL, where the map has no such key and where the stored value is NULL (LEFT JOIN);
Predicate.in_set(key, om) beside it makes the join an inner one -- a sealed map is named exactly as a set is.  The probing reader
must be opened on the map's context (`ctx=om.ctx`)."""
import ctypes as C

from . import capi
from .key_set import KeySet, check_max_keys

MAX_VALUES = 8  # ORCGPU_KEY_MAP_MAX_VALUES
LOOKUP_MAX = 8  # ORCGPU_LOOKUP_MAX
LOOKUP_MAX_PAIRS = 4
INT64, DECIMAL128, FLOAT64 = 0, 1, 2  # ORCGPU_KEY_MAP_*


def check_value_names(values, what="collect_map"):
    """The value columns of a collect: a list / tuple of 1 .. 8 non-empty str, none twice.  Returns them as a list."""
    if isinstance(values, str) or not isinstance(values, (list, tuple)):
        raise TypeError("%s: the value columns are a list of str, not %s" % (what, type(values).__name__))
    seen = set()
    for v in values:
        if not isinstance(v, str):
            raise TypeError("%s: a value column is a str, not %s" % (what, type(v).__name__))
        if not v:
            raise ValueError("%s: an empty value column name" % what)
        if v in seen:
            raise ValueError("%s: the value column %r is given twice" % (what, v))
        seen.add(v)
    if not values:
        raise ValueError("%s: no value column given" % what)
    if len(values) > MAX_VALUES:
        raise ValueError("%s: %d value columns, at most %d" % (what, len(values), MAX_VALUES))
    return list(values)


def check_collect_map_args(key, values, max_keys, into):
    """The arguments of collect_map, checked before anything reaches the GPU.  Returns the value names as a list."""
    if not isinstance(key, str):
        raise TypeError("collect_map: the key column is a str, not %s" % type(key).__name__)
    if not key:
        raise ValueError("collect_map: an empty key column name")
    values = check_value_names(values)
    check_max_keys(max_keys)
    if into is not None and not isinstance(into, KeyMap):
        raise TypeError("collect_map: into is a KeyMap, not %s" % type(into).__name__)
    if into is not None and into.sealed:
        raise ValueError("collect_map: into is sealed: it takes no further keys")
    if into is not None and into.value_names is not None and list(into.value_names) != values:
        raise ValueError("collect_map: into holds the values %r, this collect names %r" % (list(into.value_names), values))
    return values


def check_lookup_args(key_map, key, columns, ctx=None, so_far=()):
    """The arguments of with_lookup_columns, checked before anything reaches the GPU: a sealed KeyMap of the reader's context, the
    probe key column a non-empty str, `columns` a non-empty dict {output name: build value name} whose value names the map holds.
    so_far: the (map, key, name, value index) entries of earlier calls -- a (map, key) pair comes once, output names are distinct,
    at most 8 columns over at most 4 pairs.  Returns the new entries."""
    if not isinstance(key_map, KeyMap):
        raise TypeError("with_lookup_columns: the map is a KeyMap (ArrowReaderBuilder.collect_map), not %s" % type(key_map).__name__)
    if not key_map.sealed:
        raise ValueError("with_lookup_columns: the map is not sealed yet (seal() ends the build)")
    if ctx is not None and key_map.ctx is not ctx:
        raise ValueError("with_lookup_columns: the map lives on another context: open the reader with ctx=key_map.ctx")
    if not isinstance(key, str):
        raise TypeError("with_lookup_columns: the probe key column is a str, not %s" % type(key).__name__)
    if not key:
        raise ValueError("with_lookup_columns: an empty probe key column name")
    if not isinstance(columns, dict):
        raise TypeError("with_lookup_columns: columns is a dict {output name: build value name}, not %s" % type(columns).__name__)
    if not columns:
        raise ValueError("with_lookup_columns: no lookup column given")
    for m, k, _, _ in so_far:
        if m is key_map and k == key:
            raise ValueError("with_lookup_columns: the map and the probe key %r have been given already: one call per (map, key)" % key)
    names = set(n for _, _, n, _ in so_far)
    out = []
    for name, value in columns.items():
        if not isinstance(name, str) or not isinstance(value, str):
            raise TypeError("with_lookup_columns: output names and value names are str, not %s: %s" % (type(name).__name__, type(value).__name__))
        if not name:
            raise ValueError("with_lookup_columns: an empty output column name")
        if name in names:
            raise ValueError("with_lookup_columns: the output name %r is given twice" % name)
        names.add(name)
        if value not in key_map.value_names:
            raise ValueError("with_lookup_columns: the map holds no value %r (it holds %r)" % (value, list(key_map.value_names)))
        out.append((key_map, key, name, key_map.value_names.index(value)))
    if len(so_far) + len(out) > LOOKUP_MAX:
        raise ValueError("with_lookup_columns: %d lookup columns, at most %d" % (len(so_far) + len(out), LOOKUP_MAX))
    if len(set((id(m), k) for m, k, _, _ in list(so_far) + out)) > LOOKUP_MAX_PAIRS:
        raise ValueError("with_lookup_columns: more than %d (map, key) pairs" % LOOKUP_MAX_PAIRS)
    return out


def lookup_spec_array(entries):
    """(map, key, name, value index) entries -> (the orcgpu_lookup_spec array, what must stay alive beside it)."""
    arr = (capi.LookupSpec * len(entries))()
    keep = []
    for i, (m, key, name, value) in enumerate(entries):
        n, k = name.encode(), key.encode()
        keep += [n, k, m]
        arr[i].name, arr[i].key_column, arr[i].map, arr[i].value = n, k, m._h, value
    return arr, keep


class KeyMap(KeySet):
    """An open map of at most max_keys distinct keys on `ctx`'s GPU.  collect_map(..., into=this) adds to it; seal() ends the build
    -- the one host wait -- after which len(), .has_null, .rows_seen and .value_types are known, with_lookup_columns may probe it
    and Predicate.in_set may name it."""

    def __init__(self, ctx=None, max_keys=1 << 20):
        self._h = None
        check_max_keys(max_keys)
        self.ctx = ctx or capi.Context(0)
        self.max_keys = max_keys
        self._info = None
        self.value_names = None  # the value columns' names, fixed by the first collect
        h = C.c_void_p()
        self.ctx._check(self.ctx.L.orcgpu_key_map_create(self.ctx.h, max_keys, C.byref(h)))
        self._h = h.value

    def id(self):
        if not self._h:
            raise ValueError("KeyMap: the map is closed")
        return self.ctx.L.orcgpu_key_map_id(self._h)

    def seal(self):
        """Ends the build (orcgpu_key_map_seal).  More than max_keys distinct keys, or a key that came twice ("duplicate key"):
        OrcGpuError (UnsupportedTypeVariant), and the map is unusable.  Returns self."""
        if not self._h:
            raise ValueError("KeyMap: the map is closed")
        info = capi.KeyMapInfo()
        self.ctx._check(self.ctx.L.orcgpu_key_map_seal(self._h, C.byref(info)))
        self._info = info
        return self

    @property
    def value_types(self):
        """Per value column what it is stored and handed out as: "int64", "float64" or ("decimal128", precision, scale)."""
        info = self._need()
        out = []
        for k in range(info.n_values):
            kind = info.kind[k]
            out.append("int64" if kind == INT64 else "float64" if kind == FLOAT64 else ("decimal128", int(info.precision[k]), int(info.scale[k])))
        return out

    def close(self):
        """Frees the handle (orcgpu_key_map_free).  A reader that already probes the map keeps its memory until it is done."""
        if self._h:
            self.ctx.L.orcgpu_key_map_free(self._h)
            self._h = None

    def __repr__(self):
        if self._info is None:
            return "KeyMap(max_keys=%d, open)" % self.max_keys
        return "KeyMap(%d keys -> %r%s, max_keys=%d)" % (len(self), self.value_names, ", has_null" if self.has_null else "", self.max_keys)
