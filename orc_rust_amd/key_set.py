"""KeySet: the build side of a semi-join (include/orcgpu.h: orcgpu_key_set) -- the distinct non-NULL keys of one integer column
over the kept rows of one or more reads, in a hash set that stays on the GPU, and whether a kept row's key was NULL.

    keys = ArrowReaderBuilder.try_new("orders.orc").with_row_filter(...).collect_keys("o_orderkey")   # sealed
    ArrowReaderBuilder.try_new("lineitem.orc", ctx=keys.ctx).with_row_filter(Predicate.in_set("l_orderkey", keys))

    ks = KeySet(ctx, max_keys=1 << 20)                        # a build side split over files
    for f in files: ArrowReaderBuilder.try_new(f, ctx=ctx).collect_keys("k", into=ks)
    ks.seal()

The reader that probes must be opened on the set's context (`ctx=keys.ctx`)."""
import ctypes as C

from . import capi

MAX_KEYS = 1 << 26  # ORCGPU_KEY_SET_MAX_KEYS
SENTINEL = -0x7F7F7F7F7F7F7F80  # the int64 whose bytes are all 0x80: a free slot while a set is built (a legal key all the same)


def check_max_keys(max_keys):
    if isinstance(max_keys, bool) or not isinstance(max_keys, int):
        raise TypeError("max_keys: an int, not %s" % type(max_keys).__name__)
    if not 1 <= max_keys <= MAX_KEYS:
        raise ValueError("max_keys: %d is outside 1 .. 2^26" % max_keys)
    return max_keys


def check_collect_args(column, max_keys, into):
    """The arguments of collect_keys, checked before anything reaches the GPU."""
    if not isinstance(column, str):
        raise TypeError("collect_keys: the column is a str, not %s" % type(column).__name__)
    if not column:
        raise ValueError("collect_keys: an empty column name")
    check_max_keys(max_keys)
    if into is not None and not isinstance(into, KeySet):
        raise TypeError("collect_keys: into is a KeySet, not %s" % type(into).__name__)
    if into is not None and type(into) is not KeySet and hasattr(into, "value_names"):
        raise TypeError("collect_keys: into is a KeyMap: a map takes its keys with their values (collect_map)")
    if into is not None and into.sealed:
        raise ValueError("collect_keys: into is sealed: it takes no further keys")


class KeySet:
    """An open set of at most max_keys distinct keys on `ctx`'s GPU.  collect_keys(..., into=this) adds to it; seal() ends the
    build -- the one host wait -- after which len(), .has_null and .rows_seen are known and Predicate.in_set may name it."""

    def __init__(self, ctx=None, max_keys=1 << 20):
        self._h = None
        check_max_keys(max_keys)
        self.ctx = ctx or capi.Context(0)
        self.max_keys = max_keys
        self._info = None
        h = C.c_void_p()
        self.ctx._check(self.ctx.L.orcgpu_key_set_create(self.ctx.h, max_keys, C.byref(h)))
        self._h = h.value

    @property
    def sealed(self):
        return self._info is not None

    def id(self):
        if not self._h:
            raise ValueError("KeySet: the set is closed")
        return self.ctx.L.orcgpu_key_set_id(self._h)

    def seal(self):
        """Ends the build (orcgpu_key_set_seal).  More than max_keys distinct keys: OrcGpuError (UnsupportedTypeVariant) naming the
        limit, and the set is unusable.  Returns self."""
        if not self._h:
            raise ValueError("KeySet: the set is closed")
        info = capi.KeySetInfo()
        self.ctx._check(self.ctx.L.orcgpu_key_set_seal(self._h, C.byref(info)))
        self._info = info
        return self

    def _need(self):
        if self._info is None:
            raise ValueError("KeySet: not sealed yet (seal() ends the build)")
        return self._info

    def __len__(self):
        return int(self._need().n_keys)

    @property
    def has_null(self):
        return bool(self._need().has_null)

    @property
    def rows_seen(self):
        return int(self._need().rows_seen)

    def close(self):
        """Frees the handle (orcgpu_key_set_free).  A reader that already filters by the set keeps its memory until it is done."""
        if self._h:
            self.ctx.L.orcgpu_key_set_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self.ctx.h:  # (a context closed first took the library's bookkeeping with it)
                self.close()
        except Exception:
            pass

    def __repr__(self):
        if self._info is None:
            return "KeySet(max_keys=%d, open)" % self.max_keys
        return "KeySet(%d keys%s, max_keys=%d)" % (len(self), ", has_null" if self.has_null else "", self.max_keys)
