"""ORDER BY ... LIMIT k over the kept rows, selected and ordered on the GPU (include/orcgpu.h, "Top-k").  Plumbing and argument
checks only: nothing is compared here.

    from orc_rust_amd.top_k import SortKey
    table = ArrowReaderBuilder.try_new("lineitem.orc").with_row_filter(p).top_k([SortKey("l_extendedprice", descending=True)], 100)
    table = builder.top_k(["l_shipdate", ("l_extendedprice", "desc")], 10)

A sort key names a projected root column: integers, Date, Timestamp (int64 units), Boolean, Decimal, Float / Double.  `descending`
reverses the key's non-null values only; `nulls_first` places its NULLs before every value, whatever `descending` says (default:
after).  Rows equal in every key keep input order.
"""
import ctypes as C

TOP_K_MAX_KEYS = 4     # ORCGPU_TOP_K_MAX_KEYS
TOP_K_MAX = 65536      # ORCGPU_TOP_K_MAX


class SortKeyStruct(C.Structure):  # orcgpu_sort_key
    _fields_ = [("column", C.c_char_p), ("descending", C.c_uint32), ("nulls_first", C.c_uint32)]


class SortKey:
    def __init__(self, column, descending=False, nulls_first=False):
        if not isinstance(column, str):
            raise TypeError("SortKey: a column name must be a str, not %s" % type(column).__name__)
        if not column:
            raise ValueError("SortKey: an empty column name")
        for what, v in (("descending", descending), ("nulls_first", nulls_first)):
            if not isinstance(v, bool):
                raise TypeError("SortKey: %s must be a bool, not %s" % (what, type(v).__name__))
        self.column, self.descending, self.nulls_first = column, descending, nulls_first

    def __repr__(self):
        return "SortKey(%r, descending=%r, nulls_first=%r)" % (self.column, self.descending, self.nulls_first)

    def __eq__(self, other):
        return isinstance(other, SortKey) and (self.column, self.descending, self.nulls_first) == (other.column, other.descending, other.nulls_first)

    def __hash__(self):
        return hash((self.column, self.descending, self.nulls_first))


def as_key(k):
    """A SortKey, a bare str (ascending, NULLs last) or a (name, "asc" | "desc") tuple -> SortKey."""
    if isinstance(k, SortKey):
        return k
    if isinstance(k, str):
        return SortKey(k)
    if isinstance(k, tuple):
        if len(k) != 2:
            raise ValueError("top_k: a key tuple is (name, 'asc' | 'desc'), not %d items" % len(k))
        name, direction = k
        if not isinstance(direction, str):
            raise TypeError("top_k: a key's direction must be 'asc' or 'desc', not %s" % type(direction).__name__)
        if direction not in ("asc", "desc"):
            raise ValueError("top_k: a key's direction must be 'asc' or 'desc', not %r" % direction)
        return SortKey(name, descending=direction == "desc")
    raise TypeError("top_k: a sort key must be a SortKey, a str or a (name, 'asc' | 'desc') tuple, not %s" % type(k).__name__)


def check_keys(by):
    """The `by` of with_top_k / top_k, checked before anything reaches the GPU: a SortKey, str or tuple, or a list or tuple of
    1 .. 4 of them, no column twice.  Returns a list of SortKey."""
    if isinstance(by, (SortKey, str)) or (isinstance(by, tuple) and len(by) == 2 and isinstance(by[0], str) and by[1] in ("asc", "desc")):
        by = [by]
    if not isinstance(by, (list, tuple)):
        raise TypeError("top_k: `by` must be a sort key or a list or tuple of sort keys, not %s" % type(by).__name__)
    keys = [as_key(k) for k in by]
    if not keys:
        raise ValueError("top_k: no sort key given")
    if len(keys) > TOP_K_MAX_KEYS:
        raise ValueError("top_k: %d sort keys, at most %d" % (len(keys), TOP_K_MAX_KEYS))
    seen = set()
    for k in keys:
        if k.column in seen:
            raise ValueError("top_k: column %r is listed twice" % k.column)
        seen.add(k.column)
    return keys


def check_k(k):
    """k: an int (a bool is not one) in 1 .. 65536."""
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("top_k: k must be an int, not %s" % type(k).__name__)
    if k < 1 or k > TOP_K_MAX:
        raise ValueError("top_k: k must be 1 .. %d, not %d" % (TOP_K_MAX, k))
    return k


def key_array(by):
    """(the orcgpu_sort_key array of check_keys(by), what has to stay alive over the call)"""
    keys = check_keys(by)
    names = [k.column.encode() for k in keys]
    arr = (SortKeyStruct * len(keys))()
    for i, k in enumerate(keys):
        arr[i].column = names[i]
        arr[i].descending = 1 if k.descending else 0
        arr[i].nulls_first = 1 if k.nulls_first else 0
    return arr, names
