"""ArrowReaderBuilder / ArrowReader: the reference's reader API (src/arrow_reader.rs:39-347) over the
C++ host layer inside liborcgpu.so.  Pure plumbing: every call forwards to the C ABI
(`orcgpu_reader_*`), batches arrive through the Arrow C Data Interface.

    reader = ArrowReaderBuilder.try_new("file.orc").with_batch_size(8192).with_projection(["a", "b"]).build()
    for batch in reader: ...            # pyarrow.RecordBatch, like `impl Iterator<Item = Result<RecordBatch>>`
    reader = ArrowReaderBuilder.try_new("file.orc").with_device_output().build()
    for batch in reader: ...            # device_batch.DeviceRecordBatch: torch tensors over the decoder's buffers, nothing copied
"""
import ctypes as C

from . import capi

DEFAULT_BATCH_SIZE = 8192  # arrow_reader.rs:37


def check_dictionary_columns(names):
    """The argument of with_dictionary_columns, checked before anything reaches the GPU: a list or tuple of non-empty str, none
    of them twice.  Returns it as a list."""
    if not isinstance(names, (list, tuple)):
        raise ValueError("with_dictionary_columns: a list or tuple of column names, not %s" % type(names).__name__)
    seen = set()
    for n in names:
        if not isinstance(n, str):
            raise ValueError("with_dictionary_columns: a column name must be a str, not %s" % type(n).__name__)
        if not n:
            raise ValueError("with_dictionary_columns: an empty column name")
        if n in seen:
            raise ValueError("with_dictionary_columns: column %r is listed twice" % n)
        seen.add(n)
    return list(names)


COMPUTED_MAX = 8  # ORCGPU_COMPUTED_MAX


def check_computed_columns(columns):
    """The argument of with_computed_columns, checked before anything reaches the GPU: a dict {name: Expr} or a list / tuple of
    (name, Expr) pairs, 1 .. 8 of them; every name a non-empty str, none twice; every expression an orc_rust_amd.aggregate.Expr
    (col, lit, + - * / // %, divide() and year() .. extract() on them) of at most 32 nodes.  Returns the pairs as a list."""
    from .aggregate import EXPR_MAX_NODES, Expr
    if isinstance(columns, dict):
        pairs = list(columns.items())
    elif isinstance(columns, (list, tuple)):
        pairs = list(columns)
        for p in pairs:
            if not isinstance(p, (list, tuple)) or len(p) != 2:
                raise TypeError("with_computed_columns: every entry is a (name, Expr) pair, not %r" % (p,))
    else:
        raise TypeError("with_computed_columns: a dict {name: Expr} or a list of (name, Expr) pairs, not %s" % type(columns).__name__)
    seen = set()
    for name, expr in pairs:
        if not isinstance(name, str):
            raise TypeError("with_computed_columns: a column name must be a str, not %s" % type(name).__name__)
        if not name:
            raise ValueError("with_computed_columns: an empty column name")
        if name in seen:
            raise ValueError("with_computed_columns: the name %r is given twice" % name)
        seen.add(name)
        if not isinstance(expr, Expr):
            raise TypeError("with_computed_columns: the expression of %r is an aggregate.Expr (col, lit and + - * on them), not %s" % (name, type(expr).__name__))
        if expr.node_count() > EXPR_MAX_NODES:
            raise ValueError("with_computed_columns: the expression of %r has %d nodes, at most %d" % (name, expr.node_count(), EXPR_MAX_NODES))
    if not pairs:
        raise ValueError("with_computed_columns: no computed column given")
    if len(pairs) > COMPUTED_MAX:
        raise ValueError("with_computed_columns: %d computed columns, at most %d" % (len(pairs), COMPUTED_MAX))
    return [(n, e) for n, e in pairs]


def concat_batches(batches):
    """The batches of one reader as one pyarrow.Table.  (A batch's schema says "not null" of a column without a NULL in that batch,
    so the batches' schemas differ and Table.from_batches refuses them: the table is built column by column, every field nullable.)"""
    import pyarrow as pa
    names = batches[0].schema.names
    return pa.Table.from_arrays([pa.chunked_array([b.column(i) for b in batches]) for i in range(len(names))], names=names)


class ArrowReaderBuilder:
    def __init__(self, ctx, handle, keep=None):
        self._ctx, self._h, self._keep = ctx, handle, keep
        self._device_output = False

    @classmethod
    def try_new(cls, source, ctx=None):
        """source: a path (`File`) or a bytes object (`Bytes`), the two ChunkReader impls of reader/mod.rs:48-76."""
        ctx = ctx or capi.Context(0)
        out = C.c_void_p()
        if isinstance(source, (bytes, bytearray)):
            data = bytes(source)
            ctx._check(ctx.L.orcgpu_reader_open_bytes(ctx.h, data, len(data), C.byref(out)))
            return cls(ctx, out.value, data)
        ctx._check(ctx.L.orcgpu_reader_open_file(ctx.h, str(source).encode(), C.byref(out)))
        return cls(ctx, out.value)

    def with_batch_size(self, n):
        self._ctx._check(self._ctx.L.orcgpu_reader_set_batch_size(self._h, n))
        return self

    def with_projection(self, root_names):
        """ProjectionMask::named_roots (projection.rs:52-69)."""
        arr = (C.c_char_p * len(root_names))(*[n.encode() for n in root_names])
        self._ctx._check(self._ctx.L.orcgpu_reader_set_projection(self._h, arr, len(root_names)))
        return self

    def with_projection_roots(self, indices):
        """ProjectionMask::roots (projection.rs:37): root columns by index."""
        arr = (C.c_uint32 * max(1, len(indices)))(*indices)
        self._ctx._check(self._ctx.L.orcgpu_reader_set_projection_roots(self._h, arr, len(indices)))
        return self

    def with_schema(self, schema):
        """with_schema (arrow_reader.rs:80): a pyarrow.Schema, handed over through the Arrow C Data Interface."""
        buf = (C.c_uint8 * 72)()   # struct ArrowSchema
        schema._export_to_c(C.addressof(buf))
        try:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_schema(self._h, C.addressof(buf)))
        finally:
            release = C.cast(C.addressof(buf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0]  # ArrowSchema::release
            if release:
                release(C.addressof(buf))
        return self

    def with_shard(self, rank, world, mode="stripes"):
        """This reader as number `rank` of `world` readers of the same file, one per GPU (orcgpu_reader_set_shard):
        mode "stripes": stripe k belongs to rank k % world; "columns": the projected root columns dealt out by estimated Arrow bytes."""
        self._ctx._check(self._ctx.L.orcgpu_reader_set_shard(self._h, rank, world, {"stripes": 0, "columns": 1}[mode]))
        return self

    def with_file_byte_range(self, start, end):
        self._ctx._check(self._ctx.L.orcgpu_reader_set_byte_range(self._h, start, end))
        return self

    def with_timestamp_precision(self, unit):
        """unit: 'us' or 'ns' (TimestampPrecision, schema.rs:31-38); 's'/'ms' as with_schema overrides."""
        self._ctx._check(self._ctx.L.orcgpu_reader_set_timestamp_precision(self._h, {"s": 1, "ms": 2, "us": 3, "ns": 4}[unit]))
        return self

    def with_dictionary_columns(self, names):
        """The named root columns (ORC STRING / VARCHAR / CHAR) arrive as dictionary(int32, string) instead of string
        (orcgpu_reader_set_dictionary_columns): int32 keys per row and one dictionary per stripe -- the file's own where the stripe is
        dictionary-encoded, the identity dictionary where it is not.  Host batches carry pyarrow.DictionaryArrays; with
        with_device_output() a column has `values` (the keys), `validity` and `dictionary` (`offsets`, `data`)."""
        names = check_dictionary_columns(names)
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        self._ctx._check(self._ctx.L.orcgpu_reader_set_dictionary_columns(self._h, arr, len(names)))
        return self

    def with_computed_columns(self, columns):
        """Computed columns (orcgpu_reader_set_computed_columns): `columns` is a dict {name: Expr} or a list of (name, Expr), Expr
        from orc_rust_amd.aggregate (col, lit, + - *, unary -) over projected flat root columns.  Each is evaluated once per stripe
        on the GPU into an Int64, Decimal128(38, s) or Float64 column that follows the projected ones, nullable, and that the row
        filter, the aggregates, GROUP BY, top-k and collect_keys see by name.  NULL where an operand is NULL; NULL and counted
        (ArrowReader.computed_overflow_rows) where the exact value does not fit."""
        from .aggregate import AggExpr
        pairs = check_computed_columns(columns)
        names = (C.c_char_p * len(pairs))(*[n.encode() for n, _ in pairs])
        exprs = (AggExpr * len(pairs))()
        keep = []
        for i, (_, e) in enumerate(pairs):
            nodes, alive = e.flatten()
            keep.append((nodes, alive))
            exprs[i].nodes = nodes
            exprs[i].n_nodes = len(nodes)
        self._ctx._check(self._ctx.L.orcgpu_reader_set_computed_columns(self._h, names, exprs, len(pairs)))
        return self

    def with_lookup_columns(self, key_map, key, columns):
        """Lookup columns (orcgpu_reader_set_lookup_columns): `key_map` is a sealed orc_rust_amd.KeyMap on this reader's context,
        `key` the probe key (a projected Byte, Short, Int, Long or Date column of this file), `columns` a dict {output name: build
        value name}.  Each output column holds, per row, the map's value for the row's key -- NULL where the key is NULL, where the
        map has no such key and where the stored value is NULL (LEFT JOIN) --, follows the projected columns (in front of the
        computed ones), and is seen by name by the row filter, the aggregates, GROUP BY, top-k, collect_keys and collect_map.  One
        call per (map, key); up to 8 columns over up to 4 such pairs."""
        from .key_map import check_lookup_args, lookup_spec_array
        so_far = getattr(self, "_lookups", [])
        entries = so_far + check_lookup_args(key_map, key, columns, so_far=so_far)
        if key_map.ctx is not self._ctx:
            raise ValueError("with_lookup_columns: the map lives on another context: open the reader with ctx=key_map.ctx")
        arr, keep = lookup_spec_array(entries)
        self._ctx._check(self._ctx.L.orcgpu_reader_set_lookup_columns(self._h, arr, len(arr)))
        self._lookups = entries
        return self

    def with_row_selection(self, selectors):
        """RowSelection over the file's rows (arrow_reader.rs:113): selectors = [(row_count, skip)], i.e.
        RowSelector::select(n) = (n, False), RowSelector::skip(n) = (n, True)."""
        self._ctx._check(self._ctx.L.orcgpu_reader_set_row_selection(self._h, capi.selector_array(selectors), len(selectors)))
        return self

    def with_predicate(self, predicate):
        """with_predicate (arrow_reader.rs:173): a orc_rust_amd.predicate.Predicate evaluated against every stripe's row-group
        statistics and Bloom filters; only the row groups it keeps are read."""
        nodes, keep = predicate.flatten()
        self._ctx._check(self._ctx.L.orcgpu_reader_set_predicate(self._h, nodes, len(nodes)))
        return self

    def with_row_filter(self, predicate, prune=True):
        """A orc_rust_amd.predicate.Predicate evaluated on every decoded row on the GPU (orcgpu_reader_set_row_filter): only the
        rows it keeps -- SQL three-valued logic, the root must be TRUE -- are copied back and handed out, a stripe's kept rows
        packed into batches of batch_size rows.  prune=True also gives the predicate to with_predicate, so that row groups the
        statistics rule out are not read at all."""
        nodes, keep = predicate.flatten()
        self._ctx._check(self._ctx.L.orcgpu_reader_set_row_filter(self._h, nodes, len(nodes)))
        if prune:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_predicate(self._h, nodes, len(nodes)))
        return self

    def with_row_group_pruning(self, on):
        """Under a row selection, read only the row groups that hold selected rows (orcgpu_reader_set_row_group_pruning;
        default on).  The batches are the same either way."""
        self._ctx._check(self._ctx.L.orcgpu_reader_set_row_group_pruning(self._h, 1 if on else 0))
        return self

    def with_prefetch(self, stripes):
        """Read-ahead of the reader (orcgpu_reader_set_prefetch): decoded stripes it may be ahead of the consumer; 0 = none.
        The counterpart of choosing ArrowStreamReader (async_arrow_reader.rs) over ArrowReader: the batches are the same."""
        self._ctx._check(self._ctx.L.orcgpu_reader_set_prefetch(self._h, stripes))
        return self

    def with_device_output(self, on=True):
        """The reader yields device_batch.DeviceRecordBatch objects: the decoder's buffers in HBM as torch tensors, no copy to the
        host (orcgpu_reader_set_device_output).  Flat schemas only; every other builder option works as on the host path."""
        self._ctx._check(self._ctx.L.orcgpu_reader_set_device_output(self._h, 1 if on else 0))
        self._device_output = bool(on)
        return self

    def aggregate(self, specs, raw=False, group_by=None, max_groups=None, max_total_groups=None):
        """COUNT, SUM, AVG, MIN, MAX, SUM(a * b) and SUM / AVG of an arithmetic expression (aggregate.col / aggregate.lit) over the rows the builder's selection and row filter keep -- each aggregate over its own subset of them when it carries a condition (Agg.where) --, reduced on the GPU
        (orcgpu_reader_set_aggregates / orcgpu_reader_aggregate): specs is a list of orc_rust_amd.aggregate.Agg, the result a list
        of int (counts, integer results; a Timestamp's with `.units`), decimal.Decimal, float, or None for NULL.  Builds the reader
        and drains it: every stripe is decoded and aggregated where it lies, no batch is copied back.  The projection must hold the
        aggregated and the filter's columns.  OverflowError, naming the spec, when a result leaves its range.

        group_by: a list or tuple of 1 .. 4 distinct column names (orcgpu_reader_set_group_by / orcgpu_reader_aggregate_groups): the
        result is a list of (keys tuple, values list), one per group of kept rows, in order of first appearance; at most 256
        groups a stripe.  A key is an int, bool, decimal.Decimal, str (bytes when not UTF-8) or None for the NULL key.  The
        projection must hold the key columns too.  OverflowError names the spec and the group's keys.

        max_groups (1 .. 2^20) and max_total_groups (1 .. 2^24, not below max_groups) raise the limits of groups in one stripe and
        over the file from 256 and 65536 (orcgpu_reader_set_group_limits); they need group_by.  A max_groups above 256 runs the
        wide path -- a sort of the kept rows by group and a segmented reduction -- for every stripe, however few groups it holds:
        GROUP BY l_suppkey, l_partkey.  A Float sum may differ in its last bits from the default path's."""
        return self.aggregating_reader(specs, group_by=group_by, max_groups=max_groups, max_total_groups=max_total_groups).aggregate(raw=raw)

    def aggregating_reader(self, specs, group_by=None, max_groups=None, max_total_groups=None):
        """The same in two steps: the ArrowReader whose aggregate() drains it (and whose filter_rows() / d2h_bytes() report on it)."""
        from . import aggregate as A
        max_groups, max_total_groups = A.check_group_limits(max_groups, max_total_groups, group_by)
        arr, keep = A.spec_array(specs)
        keys = A.key_array(group_by) if group_by is not None else None
        exprs, keep_e = A.expr_array(specs)
        if exprs is None:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_aggregates(self._h, arr, len(arr)))
        else:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_aggregate_exprs(self._h, arr, exprs, len(arr)))
        filters, keep_f = A.filter_array(specs)
        if filters is not None:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_aggregate_filters(self._h, filters, len(arr)))
        if keys is not None:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_group_by(self._h, keys, len(keys)))
        if max_groups or max_total_groups:
            self._ctx._check(self._ctx.L.orcgpu_reader_set_group_limits(self._h, max_groups, max_total_groups))
        r = self.build()
        r._agg_specs = A.check_specs(specs)
        r._group_by = A.check_group_by(group_by) if group_by is not None else None
        return r

    def collect_keys(self, column, max_keys=1 << 20, into=None):
        """The build side of a semi-join (orcgpu_reader_collect_keys): builds the reader and drains it -- every stripe is decoded,
        the builder's row selection and row filter are applied as a keep mask, and the kept rows' distinct non-NULL keys of `column`
        (a projected Byte, Short, Int, Long or Date column) go into a hash set that stays on the GPU; no batch is copied back.
        Returns the orc_rust_amd.KeySet, sealed, for Predicate.in_set; max_keys (1 .. 2^26) fixes its capacity, and more distinct
        keys than that fail the seal.  into: a KeySet that is still open (KeySet(ctx, max_keys)) -- the keys are added to it and it
        is left open, so that several files can build one set; seal() it afterwards."""
        from .key_set import KeySet, check_collect_args
        check_collect_args(column, max_keys, into)
        ks = into if into is not None else KeySet(self._ctx, max_keys)
        reader = self.build()
        try:
            reader.collect_keys(column, ks)
            if into is None:
                ks.seal()
        except Exception:
            if into is None:
                ks.close()
            raise
        finally:
            reader.close()
        return ks

    def collect_map(self, key, values, max_keys=1 << 20, into=None):
        """The build side of a many-to-one join (orcgpu_reader_collect_map): builds the reader and drains it as collect_keys does;
        the kept rows' non-NULL keys of `key` go into a hash table on the GPU and, beside each, the row's values of the columns
        `values` (1 .. 8 projected Byte .. Long, Date, Decimal, Float or Double columns -- computed and lookup columns of this
        reader among them).  The keys must be unique: a key that comes twice fails the seal ("duplicate key").  Returns the
        orc_rust_amd.KeyMap, sealed, for with_lookup_columns and Predicate.in_set.  into: a KeyMap that is still open -- it is left
        open, so that several files can build one map; seal() it afterwards."""
        from .key_map import KeyMap, check_collect_map_args
        values = check_collect_map_args(key, values, max_keys, into)
        km = into if into is not None else KeyMap(self._ctx, max_keys)
        reader = self.build()
        try:
            reader.collect_map(key, values, km)
            if into is None:
                km.seal()
        except Exception:
            if into is None:
                km.close()
            raise
        finally:
            reader.close()
        return km

    def with_top_k(self, by, k):
        """ORDER BY by LIMIT k (orcgpu_reader_set_top_k): `by` is a list of orc_rust_amd.top_k.SortKey (a bare column name and a
        (name, "asc" | "desc") tuple are accepted for one).  The reader then iterates every stripe's own at most k best kept rows,
        sorted, selected on the GPU behind the row selection and the row filter; ArrowReader.top_k_order() merges them once the
        reader is drained.  Not together with aggregates."""
        from . import top_k as T
        keys, keep = T.key_array(by)
        self._ctx._check(self._ctx.L.orcgpu_reader_set_top_k(self._h, keys, len(keys), T.check_k(k)))
        return self

    def top_k(self, by, k):
        """The same, drained: one pyarrow.Table of the answer in order -- the stripes' candidates concatenated, then one `take` by
        ArrowReader.top_k_order().  Host output."""
        import pyarrow as pa
        reader = self.with_top_k(by, k).build()
        batches = list(reader)
        order = reader.top_k_order()
        if not batches:  # (no kept row: no batch, so no schema -- the projected names over null columns)
            return pa.schema([(n, pa.null()) for n in reader.column_names()]).empty_table()
        return concat_batches(batches).take(pa.array(order, type=pa.uint64()))

    def total_row_count(self):
        return self._ctx.L.orcgpu_reader_total_rows(self._h)

    def stripe_count(self):
        return self._ctx.L.orcgpu_reader_stripe_count(self._h)

    def build(self):
        r = ArrowReader(self._ctx, self._h, self._keep, self._device_output)
        self._h = None
        return r

    def __del__(self):
        if getattr(self, "_h", None):
            self._ctx.L.orcgpu_reader_close(self._h)


class ArrowReader:
    def __init__(self, ctx, handle, keep=None, device_output=False):
        self._ctx, self._h, self._keep = ctx, handle, keep
        self._device_output = device_output

    def total_row_count(self):
        return self._ctx.L.orcgpu_reader_total_rows(self._h)

    def row_groups(self):
        """(row groups read so far, row groups of the stripes gone through so far): orcgpu_reader_row_groups."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ctx._check(self._ctx.L.orcgpu_reader_row_groups(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def filter_rows(self):
        """(rows the row filter has seen so far, rows it has kept): orcgpu_reader_filter_rows."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ctx._check(self._ctx.L.orcgpu_reader_filter_rows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def filter_overflow_rows(self):
        """(row, expression leaf) evaluations of the row filter so far in which an operation inside a side of a Predicate.compare
        leaf left 128 bits -- the leaf was UNKNOWN there: orcgpu_reader_filter_overflow_rows.  0 unless something overflowed."""
        n = C.c_uint64(0)
        self._ctx._check(self._ctx.L.orcgpu_reader_filter_overflow_rows(self._h, C.byref(n)))
        return n.value

    def computed_overflow_rows(self):
        """Rows decoded so far in which a computed column's value did not fit -- an operation left 128 bits, an Int64 result left
        int64, a Decimal result reached 10^38 -- and is NULL: orcgpu_reader_computed_overflow_rows.  0 unless something overflowed."""
        n = C.c_uint64(0)
        self._ctx._check(self._ctx.L.orcgpu_reader_computed_overflow_rows(self._h, C.byref(n)))
        return n.value

    def d2h_bytes(self):
        """Column-buffer bytes this reader has copied to the host so far (orcgpu_reader_d2h_bytes); 0 with device output."""
        n = C.c_uint64(0)
        self._ctx._check(self._ctx.L.orcgpu_reader_d2h_bytes(self._h, C.byref(n)))
        return n.value

    def top_k_order(self):
        """Once the reader is drained: where the rows of the global answer of with_top_k stand in the concatenation of all rows it
        handed out, in order (orcgpu_reader_top_k_order) -- a list of ints, min(k, kept rows) long."""
        n = C.c_uint64(0)
        rc = self._ctx.L.orcgpu_reader_top_k_order(self._h, None, 0, C.byref(n))
        if rc and not n.value:
            self._ctx._check(rc)
        out = (C.c_uint64 * max(1, n.value))()
        self._ctx._check(self._ctx.L.orcgpu_reader_top_k_order(self._h, out, n.value, C.byref(n)))
        return list(out)[:n.value]

    def aggregate(self, raw=False):
        """Drains a reader built by ArrowReaderBuilder.aggregating_reader (orcgpu_reader_aggregate): the list of Python values."""
        from . import aggregate as A
        specs = getattr(self, "_agg_specs", None)
        if getattr(self, "_group_by", None) is not None:
            handle = C.c_void_p()
            rc = self._ctx.L.orcgpu_reader_aggregate_groups(self._h, C.byref(handle))
            if rc == 110:
                raise StopIteration
            self._ctx._check(rc)
            return A.groups_of(self._ctx.L, handle, len(self._group_by), specs, raw=raw)
        out = (A.AggValue * max(1, len(specs or ())))()
        rc = self._ctx.L.orcgpu_reader_aggregate(self._h, out)
        if rc == 110:  # ORCGPU_END_OF_FILE: the reader has been drained before
            raise StopIteration
        self._ctx._check(rc)
        return list(out)[:len(specs)] if raw else A.values_of(out, specs)

    def collect_map(self, key, values, key_map):
        """Drains this reader into an open KeyMap (orcgpu_reader_collect_map): what ArrowReaderBuilder.collect_map does, for a
        reader built by hand."""
        from .key_map import check_collect_map_args
        values = check_collect_map_args(key, values, key_map.max_keys if hasattr(key_map, "max_keys") else 1, key_map)
        va = (C.c_char_p * len(values))(*[v.encode() for v in values])
        self._ctx._check(self._ctx.L.orcgpu_reader_collect_map(self._h, key.encode(), va, len(values), key_map._h))
        key_map.value_names = values
        return key_map

    def collect_keys(self, column, key_set):
        """Drains this reader into an open KeySet (orcgpu_reader_collect_keys): what ArrowReaderBuilder.collect_keys does, for a
        caller that wants the reader's filter_rows() / d2h_bytes() afterwards.  The set is left open."""
        from .key_set import check_collect_args
        check_collect_args(column, key_set.max_keys if hasattr(key_set, "max_keys") else 1, key_set)
        self._ctx._check(self._ctx.L.orcgpu_reader_collect_keys(self._h, column.encode(), key_set._h))
        return key_set

    def reads_ahead(self):
        """Whether the reader's read-ahead threads are at work on its context right now (orcgpu_reader_reads_ahead)"""
        return bool(self._h) and bool(self._ctx.L.orcgpu_reader_reads_ahead(self._h))

    def column_names(self):
        n = self._ctx.L.orcgpu_reader_column_count(self._h)
        return [self._ctx.L.orcgpu_reader_column_name(self._h, i).decode() for i in range(n)]

    def __iter__(self):
        return self

    def _next_device(self):
        import pyarrow as pa
        from .device_batch import ArrowDeviceArrayStruct, DeviceRecordBatch
        a = ArrowDeviceArrayStruct()
        s = (C.c_uint8 * 72)()
        rc = self._ctx.L.orcgpu_reader_next_batch_device(self._h, C.addressof(a), C.addressof(s))
        if rc == 110:  # ORCGPU_END_OF_FILE
            raise StopIteration
        self._ctx._check(rc)
        return DeviceRecordBatch(self._ctx, a, pa.Schema._import_from_c(C.addressof(s)), self)

    def __next__(self):
        import pyarrow as pa
        if self._device_output:
            return self._next_device()
        a = (C.c_uint8 * 80)()
        s = (C.c_uint8 * 72)()
        rc = self._ctx.L.orcgpu_reader_next_batch(self._h, C.addressof(a), C.addressof(s))
        if rc == 110:  # ORCGPU_END_OF_FILE
            raise StopIteration
        self._ctx._check(rc)
        return pa.RecordBatch._import_from_c(C.addressof(a), C.addressof(s))

    def close(self):
        if self._h:
            self._ctx.L.orcgpu_reader_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
