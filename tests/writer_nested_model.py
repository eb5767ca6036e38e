"""ArrowWriter's Struct, List and Map columns restated in Python over writer_model's encoder state machines, writer_types_model's
Timestamp / Decimal128 columns and the oracle's encoders: the bytes of the file the writer writes for a nested schema.

The column tree is the ORC type tree in preorder (column 0 the root): a Struct is STRUCT (12), a List / LargeList LIST (10), a Map
MAP (11) whose two children are its key and value (the Arrow entries struct gets no column).  ORC stores for each column one
entry per existing row of its parent, so a node's `encode(array, idx)` takes the Arrow array of its column and the logical rows
of it that are its ORC rows: a Struct hands its valid rows on, a List the ranges of its valid rows one behind the other -- a
null list that owns a range contributes nothing, the array's own offset and length are honoured at every level.  PRESENT follows
the flat columns' sticky rule (writer/column.rs:103-139), per column, over its ORC rows: it begins, back-filled with ones, when
an array of the column with a validity buffer arrives (whatever the rows of it in the slice).

Streams, by column id: Struct [PRESENT] (DIRECT); List / Map LENGTH, [PRESENT] (DIRECT_V2; the lengths of the valid rows,
unsigned RLE v2 in the offsets' width); leaves as the flat writer.  The stripe cut is the reference's over root rows: after each
slice of batch_size root rows the estimates of all columns of the tree are summed and compared with stripe_byte_size.

Not written (NotImplementedError, naming the field's path): FixedSizeList, ListView, Union, dictionary and run-end encoded
types, Decimal128 below a List or Map, and every leaf the flat writer lacks."""
import numpy as np
import pyarrow as pa

import oracle_lib as O
import writer_model as WM
import writer_types_model as TM

T = pa.types


def _no_bitmap(arr):
    return pa.Array.from_buffers(arr.type, len(arr), [None] + arr.buffers()[1:], offset=arr.offset)


class Node:
    """a column of the tree; `out`: the preorder list it joins (its id: its place + 1)"""

    def __init__(self, field, path, under_list, out):
        t = field.type
        self.name, self.path, self.type, self.kids, self.leaf = field.name, path, t, [], None
        out.append(self)
        self.id = len(out)
        self.present = None
        if T.is_struct(t):
            self.w, self.orc_kind, self.encoding, self.ob = "struct", 12, 0, 0
            sub = [t.field(i) for i in range(t.num_fields)]
        elif T.is_map(t):
            self.w, self.orc_kind, self.encoding, self.ob = "list", 11, 2, 4
            sub, under_list = [t.key_field, t.item_field], True
        elif T.is_list(t) or T.is_large_list(t):
            self.w, self.orc_kind, self.encoding, self.ob = "list", 10, 2, 8 if T.is_large_list(t) else 4
            sub, under_list = [t.value_field], True
        else:
            sub = []
            if T.is_nested(t) or T.is_dictionary(t) or T.is_run_end_encoded(t) or (T.is_decimal128(t) and under_list):
                raise NotImplementedError("unsupported datatype %s of field %s" % (t, path))
            try:
                self.leaf = TM.ColumnModel(field) if TM.is_new(t) else WM.ColumnModel(field)
            except NotImplementedError:
                raise NotImplementedError("unsupported datatype %s of field %s" % (t, path))
            self.w, self.orc_kind, self.encoding = "leaf", self.leaf.orc_kind, self.leaf.encoding
        for f in sub:
            self.kids.append(Node(f, path + "." + f.name, under_list, out))
        self.reset()

    def reset(self):
        if self.leaf is not None:
            self.leaf.reset()
            return
        self.lengths, self.n_present = [], 0
        self.enc = WM.RleV2Model(self.ob, False) if self.w == "list" else None
        if self.present is not None:
            self.present = []

    def children_of(self, arr):
        """(Arrow arrays of the children, offsets or None): a Struct's children carry its offset; a List's / Map's are whole"""
        if self.w == "struct":
            return [arr.field(i) for i in range(len(self.kids))], None
        offs = np.asarray(arr.offsets).astype(np.int64)
        kids = [arr.keys, arr.items] if T.is_map(self.type) else [arr.values]
        if len(offs) and (offs[0] < 0 or np.any(np.diff(offs) < 0) or offs[-1] > min(len(k) for k in kids)):
            raise ValueError("offsets of %s descend or address rows beyond the child" % self.path)
        return kids, offs

    def walk(self, arr, idx, visit):
        """visit(node, arr, idx) for this column and those below, without changing anything (validation)"""
        visit(self, arr, idx)
        if self.leaf is not None:
            return
        kids, offs = self.children_of(arr)
        kidx = self.child_rows(arr, idx, offs)[0]
        for k, a in zip(self.kids, kids):
            k.walk(a, kidx, visit)

    def child_rows(self, arr, idx, offs):
        valid = np.ones(len(idx), dtype=bool) if arr.buffers()[0] is None else np.asarray(arr.is_valid())[idx]
        keep = idx[valid]
        if offs is None:
            return keep, valid, None
        lens = offs[keep + 1] - offs[keep]
        kidx = np.concatenate([np.arange(offs[i], offs[i + 1], dtype=np.int64) for i in keep] + [np.zeros(0, dtype=np.int64)])
        return kidx, valid, lens

    def encode(self, arr, idx):
        has_bitmap = arr.buffers()[0] is not None
        if self.leaf is not None:
            c = self.leaf
            if has_bitmap and c.present is None:
                c.present = [1] * c.n_present
            sub = arr.take(pa.array(idx, type=pa.int64()))
            c.encode_array(sub if has_bitmap else _no_bitmap(sub))
            return
        kids, offs = self.children_of(arr)
        kidx, valid, lens = self.child_rows(arr, idx, offs)
        if has_bitmap and self.present is None:
            self.present = [1] * self.n_present
        if self.present is not None:
            self.present.extend(valid.astype(np.uint8).tolist())
        self.n_present += len(idx)
        if lens is not None:
            for v in lens.tolist():
                self.lengths.append(v)
                self.enc.push(v)
        for k, a in zip(self.kids, kids):
            k.encode(a, kidx)

    def estimate(self):
        if self.leaf is not None:
            return self.leaf.estimate()
        e = self.enc.estimate() if self.enc is not None else 0
        return e + (len(self.present) // 8 if self.present is not None else 0)

    def finish(self):
        if self.leaf is not None:
            return self.leaf.finish()
        out = []
        if self.w == "list":
            v = np.array(self.lengths, dtype=np.int64)
            data = O.enc_rle2(v, self.ob, False) if len(v) else b""
            assert b"".join(self.enc.runs) + self.enc.finish() == data
            out.append((2, data))
        if self.present is not None:
            p = np.array(self.present, dtype=np.uint8)
            out.append((0, O.enc_boolean(np.packbits(p, bitorder="little"), len(p)) if len(p) else b""))
        return out


def _check_timestamps(node, arr, idx):
    if node.leaf is not None and T.is_timestamp(node.type):
        for v in TM.timestamp_ints(arr.take(pa.array(idx, type=pa.int64()))):
            TM.ts_stored(*TM.ts_split(v, node.type.unit))


class WriterModel(TM.WriterModel):
    def __init__(self, schema, batch_size=1024, stripe_byte_size=64 << 20):
        self.schema, self.bs, self.sbs = schema, batch_size, stripe_byte_size
        self.cols = []  # preorder: flush_stripe writes the streams and encodings in this order
        self.roots = [Node(f, f.name, False, self.cols) for f in schema]
        self.out = bytearray(b"ORC")
        self.stripes = []
        self.rows = 0
        self.has_ts = any(c.leaf is not None and T.is_timestamp(c.type) for c in self.cols)

    def write(self, batch):
        """a batch with bad offsets or a value that has no encoding changes nothing (ValueError)"""
        if not batch.schema.equals(self.schema, check_metadata=True):
            raise ValueError("RecordBatch doesn't match expected schema")
        n = batch.num_rows
        if n == 0:
            return
        every = np.arange(n, dtype=np.int64)
        for r, arr in zip(self.roots, batch.columns):
            r.walk(arr, every, _check_timestamps)
        for off in range(0, n, self.bs):
            idx = np.arange(off, min(off + self.bs, n), dtype=np.int64)
            for r, arr in zip(self.roots, batch.columns):
                r.encode(arr, idx)
            self.rows += len(idx)
            if self.estimate() > self.sbs:
                self.flush_stripe()

    def close(self):
        if self.rows > 0:
            self.flush_stripe()
        f = WM._Pb()
        f.u64(1, 3)
        f.u64(2, sum(s[1] + s[2] for s in self.stripes) + 3)
        for off, dl, fl, rows in self.stripes:
            m = WM._Pb()
            for k, v in enumerate((off, 0, dl, fl, rows)):
                m.u64(k + 1, v)
            f.bytes(3, bytes(m.b))
        root = WM._Pb()
        root.u64(1, 12)
        root.packed(2, [r.id for r in self.roots])
        for r in self.roots:
            root.bytes(3, r.name.encode())
        f.bytes(4, bytes(root.b))
        for c in self.cols:
            t = WM._Pb()
            t.u64(1, c.orc_kind)
            t.packed(2, [k.id for k in c.kids])
            if c.w == "struct":
                for k in c.kids:
                    t.bytes(3, k.name.encode())
            if c.orc_kind == 14:
                t.u64(5, c.type.precision)
                t.u64(6, c.type.scale)
            f.bytes(4, bytes(t.b))
        f.u64(6, sum(s[3] for s in self.stripes))
        f.u64(9, 0xFFFFFFFF)
        ps = WM._Pb()
        ps.u64(1, len(f.b))
        ps.u64(2, 0)
        ps.packed(4, [0, 12])
        ps.u64(5, 0)
        ps.u64(6, 0xFFFFFFFF)
        ps.bytes(8000, b"ORC")
        self.out += f.b + ps.b + bytes([len(ps.b)])
        return bytes(self.out)


def write_model(batches, schema=None, batch_size=1024, stripe_byte_size=64 << 20, flush_after=()):
    """as writer_types_model.write_model: the file's bytes and its stripes' rows; a rejected batch is skipped"""
    m = WriterModel(schema or batches[0].schema, batch_size, stripe_byte_size)
    for i, b in enumerate(batches):
        try:
            m.write(b)
        except ValueError:
            pass
        if i in flush_after:
            m.flush_stripe()
    data = m.close()
    return data, m.stripe_rows()


def read_type(t):
    """the type a column reads back as: TIMESTAMP as Timestamp(ns), the large types as the small, at every level"""
    if T.is_timestamp(t):
        return pa.timestamp("ns", "UTC" if t.tz else None)
    if T.is_struct(t):
        return pa.struct([pa.field(t.field(i).name, read_type(t.field(i).type)) for i in range(t.num_fields)])
    if T.is_map(t):
        return pa.map_(read_type(t.key_type), read_type(t.item_type))
    if T.is_list(t) or T.is_large_list(t):
        return pa.list_(read_type(t.value_type))
    return {pa.large_string(): pa.string(), pa.large_binary(): pa.binary()}.get(t, t)


def read_types(table):
    return table.cast(pa.schema([pa.field(f.name, read_type(f.type)) for f in table.schema]))


# ---- the tables the tests of the model and of the device writer share ---------------------------------------------------------
def list_array(n, rng, value, nulls=0.0, empties=0.2, large=False, max_len=5, null_ranges=True):
    """a List array of n rows over value(count) -> child array; null lists own non-empty ranges when null_ranges"""
    lens = rng.integers(0, max_len + 1, n)
    lens[rng.random(n) < empties] = 0
    mask = rng.random(n) < nulls if nulls else np.zeros(n, dtype=bool)
    if not null_ranges:
        lens[mask] = 0
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64 if large else np.int32)
    child = value(int(offs[-1]))
    t = pa.large_list(child.type) if large else pa.list_(child.type)
    bufs = [None if not nulls else pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes()), pa.py_buffer(offs.tobytes())]
    return pa.Array.from_buffers(t, n, bufs, children=[child], null_count=-1)


def ints(rng, dtype=np.int32, nulls=0.0):
    def make(n):
        v = rng.integers(-1000, 1000, n).astype(dtype)
        return pa.array(v, mask=(rng.random(n) < nulls) if nulls else None)
    return make


def strings(rng, nulls=0.0, binary=False):
    def make(n):
        v = [("s%d" % x) * int(x % 4) for x in rng.integers(0, 50, n)]
        v = [x.encode() for x in v] if binary else v
        return pa.array(v, type=pa.binary() if binary else pa.string(), mask=(rng.random(n) < nulls) if nulls else None)
    return make


def map_array(keys, items):
    """a Map with the validity and offsets of the List array `keys` (over the keys) and `items` beside its values"""
    t = pa.map_(keys.type.value_type, items.type)
    entries = pa.StructArray.from_arrays([keys.values, items], fields=[t.key_field, t.item_field])
    return pa.Array.from_buffers(t, len(keys), keys.buffers()[:2], children=[entries], null_count=-1, offset=keys.offset)


def raw_list(offsets, child, large=False):
    """a List array over `child` with these offsets, whatever those between the first and the last say (pyarrow checks the two ends)"""
    o = np.asarray(offsets, dtype=np.int64 if large else np.int32)
    return pa.Array.from_buffers(pa.large_list(child.type) if large else pa.list_(child.type), len(o) - 1, [None, pa.py_buffer(o.tobytes())], children=[child])


def expected_paths(arr):
    """(gathers, slices) of the one child of a top-level List array: a slice unless a null list owns a non-empty range"""
    offs, valid = np.asarray(arr.offsets).astype(np.int64), np.asarray(arr.is_valid())
    lens = np.diff(offs)
    if lens[valid].sum() == 0:
        return 0, 0
    return (1, 0) if np.any(lens[~valid] > 0) else (0, 1)
