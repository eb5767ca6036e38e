"""ArrowWriter's string dictionaries (orcgpu_writer_set_dictionary, ArrowWriterBuilder.with_dictionary_key_size_threshold)
restated in Python over writer_model / writer_nested_model (the container, the stripe cut, the direct streams) and index_model
(the row index): the bytes of the whole file for a list of batches, a threshold and the other builder options.

The rule, per stripe and per Utf8 / LargeUtf8 column, at any depth of the column tree: with n the column's non-null ORC rows in
the stripe and d the distinct byte strings among them, the column is DICTIONARY_V2 in that stripe iff n > 0 and
float(d) <= t * float(n).  Then its streams are DATA (the rows' ids, unsigned RLE v2 in the offsets' width), LENGTH (the
entries' lengths, likewise), DICTIONARY_DATA (the entries' bytes back to back), [PRESENT], and its ColumnEncoding is
{DICTIONARY_V2, dictionary_size d}; entry k is the k-th distinct value in row order.  Else the column's streams and encoding are
the direct ones.  The stripe cut is writer_model's over the direct encoders' estimates, whatever the threshold.

With a row index stride (flat schemas of integers, strings and binaries here: their statistics are exact) the entries of a
dictionary column hold [PRESENT's positions,] then the run-length positions of DATA's ids, nothing for LENGTH or
DICTIONARY_DATA."""
import numpy as np
import pyarrow as pa

import index_model as IM
import oracle_lib as O
import writer_model as WM
import writer_nested_model as NM

DICTIONARY_V2 = 3


def is_dictionary(n, d, t):
    """the key-ratio rule, in double arithmetic"""
    return t > 0 and n > 0 and float(d) <= t * float(n)


def dictionary_of(strs):
    """(entries in first-occurrence order, the rows' ids)"""
    ids, entries, seen = [], [], {}
    for s in strs:
        k = seen.get(s)
        if k is None:
            k = seen[s] = len(entries)
            entries.append(s)
        ids.append(k)
    return entries, ids


def _is_string_leaf(node):
    return node.leaf is not None and node.orc_kind == 7


def _zz(v):
    return (v << 1) ^ (v >> 63)


def _stats_msg(d):
    """index_model's statistics dict -> ColumnStatistics"""
    m = WM._Pb()
    m.u64(1, d["n"])
    t = WM._Pb()
    if "int" in d:
        mn, mx, s = d["int"]
        t.u64(1, _zz(mn))
        t.u64(2, _zz(mx))
        if s is not None:
            t.u64(3, _zz(s))
        m.bytes(2, bytes(t.b))
    elif "string" in d:
        mn, mx, lo, up, s = d["string"]
        if mn is not None:
            t.bytes(1, mn)
        if mx is not None:
            t.bytes(2, mx)
        t.u64(3, _zz(s))
        if lo is not None:
            t.bytes(4, lo)
        if up is not None:
            t.bytes(5, up)
        m.bytes(4, bytes(t.b))
    elif "binary" in d:
        t.u64(1, _zz(d["binary"]))
        m.bytes(8, bytes(t.b))
    elif "bucket" in d:
        t.packed(1, d["bucket"])
        m.bytes(5, bytes(t.b))
    elif "double" in d:
        raise NotImplementedError("float statistics are not exact: no byte model of their row index")
    m.u64(10, 1 if d["has_null"] else 0)
    return bytes(m.b)


class WriterModel(NM.WriterModel):
    def __init__(self, schema, batch_size=1024, stripe_byte_size=64 << 20, threshold=0.0, row_index_stride=0):
        super().__init__(schema, batch_size, stripe_byte_size)
        t = float(threshold)
        if isinstance(threshold, bool) or t != t or t < 0 or t > 1:
            raise ValueError("threshold must be in 0 .. 1")
        self.t, self.stride = t, row_index_stride
        self.n_dictionary = self.n_direct = 0
        self.stripes = []  # (offset, data_length, footer_length, rows, index_length)
        self.decisions = []  # per stripe: {column id: dictionary size or None (direct)} of the string columns
        self.parts = [[] for _ in self.cols]  # row index: the stripe's rows of each (flat) column
        self.all_parts = [[] for _ in self.cols]
        self.stripe_stats = []
        if self.stride and any(c.leaf is None for c in self.cols):
            raise NotImplementedError("no row index for a nested schema")

    def write(self, batch):
        if not self.stride:
            return super().write(batch)
        if not batch.schema.equals(self.schema, check_metadata=True):
            raise ValueError("RecordBatch doesn't match expected schema")
        n = batch.num_rows
        for off in range(0, n, self.bs):
            sl = batch.slice(off, min(self.bs, n - off))
            idx = np.arange(off, off + sl.num_rows, dtype=np.int64)
            for i, (r, arr) in enumerate(zip(self.roots, batch.columns)):
                r.encode(arr, idx)
                self.parts[i].append(sl.column(i))
            self.rows += sl.num_rows
            if self.estimate() > self.sbs:
                self.flush_stripe()

    def _streams_of(self, c, decisions):
        streams, enc = c.finish(), (c.encoding, None)
        ids = None
        if _is_string_leaf(c):
            strs = c.leaf.strs
            entries, ids = dictionary_of(strs)
            if is_dictionary(len(strs), len(entries), self.t):
                ob = c.leaf.ob
                present = [s for s in streams if s[0] == 0]
                streams = [(1, O.enc_rle2(np.array(ids, dtype=np.int64), ob, False)),
                           (2, O.enc_rle2(np.array([len(e) for e in entries], dtype=np.int64), ob, False)),
                           (3, b"".join(entries))] + present
                enc = (DICTIONARY_V2, len(entries))
                self.n_dictionary += 1
                decisions[c.id] = len(entries)
            else:
                self.n_direct += 1
                decisions[c.id] = None
                ids = None
        return streams, enc, ids

    def _index(self, col_streams):
        """the ROW_INDEX streams of the stripe (column 0 first), and its statistics"""
        S, out = self.stride, []
        root = WM._Pb()
        for r0 in range(0, self.rows, S):
            e = WM._Pb()
            e.bytes(2, _stats_msg(IM.root_stats(min(S, self.rows - r0))))
            root.bytes(1, bytes(e.b))
        out.append(bytes(root.b))
        stats = [IM.root_stats(self.rows)]
        for i, c in enumerate(self.cols):
            parts = [p for p in self.parts[i] if len(p)]
            arr = pa.concat_arrays(parts) if parts else pa.array([], type=c.type)
            has_present = c.leaf.present is not None
            _, enc, ids = col_streams[i]
            if enc[0] == DICTIONARY_V2 and _is_string_leaf(c):
                valid = np.asarray(arr.is_valid()).astype(np.uint8)
                before = np.concatenate([[0], np.cumsum(valid)])
                ptab = IM.RunTable(IM.ByteRuns(), IM.msb_bytes(valid)) if has_present else None
                dtab = IM.RunTable(IM.Rle2Runs(c.leaf.ob, False), ids)
                positions = []
                for r0 in range(0, self.rows, S):
                    pos = []
                    if has_present:
                        u, cons = ptab.at(r0 // 8)
                        pos += [u, cons, r0 % 8]
                    pos += list(dtab.at(int(before[r0])))
                    positions.append(pos)
            else:
                positions = IM.model_positions(arr, has_present, S)
            ri = WM._Pb()
            for g, r0 in enumerate(range(0, self.rows, S)):
                e = WM._Pb()
                e.packed(1, positions[g])
                e.bytes(2, _stats_msg(IM.column_stats(arr.slice(r0, min(S, self.rows - r0)))))
                ri.bytes(1, bytes(e.b))
            out.append(bytes(ri.b))
            stats.append(IM.column_stats(arr))
            self.all_parts[i] += parts
        self.stripe_stats.append(stats)
        self.parts = [[] for _ in self.cols]
        return out

    def flush_stripe(self):
        start = len(self.out)
        decisions = {}
        col_streams = [self._streams_of(c, decisions) for c in self.cols]
        index = self._index(col_streams) if self.stride else []
        for b in index:
            self.out += b
        streams, data_len = [], 0
        for i, (st, _, _) in enumerate(col_streams):
            for kind, b in st:
                self.out += b
                data_len += len(b)
                streams.append((kind, i + 1, len(b)))
        f = WM._Pb()
        for kind, col, ln in [(6, ci, len(b)) for ci, b in enumerate(index)] + streams:
            m = WM._Pb()
            m.u64(1, kind)
            m.u64(2, col)
            m.u64(3, ln)
            f.bytes(1, bytes(m.b))
        for kind, dsz in [(0, None)] + [e for _, e, _ in col_streams]:
            m = WM._Pb()
            m.u64(1, kind)
            if dsz is not None:
                m.u64(2, dsz)
            f.bytes(2, bytes(m.b))
        if self.has_ts:
            f.bytes(3, b"UTC")
        self.out += f.b
        self.stripes.append((start, data_len, len(f.b), self.rows, sum(len(b) for b in index)))
        self.decisions.append(decisions)
        self.rows = 0
        for c in self.cols:
            c.reset()

    def close(self):
        if self.rows > 0:
            self.flush_stripe()
        f = WM._Pb()
        f.u64(1, 3)
        f.u64(2, sum(s[1] + s[2] + s[4] for s in self.stripes) + 3)
        for off, dl, fl, rows, il in self.stripes:
            m = WM._Pb()
            for k, v in enumerate((off, il, dl, fl, rows)):
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
        total = sum(s[3] for s in self.stripes)
        f.u64(6, total)
        md = WM._Pb()
        if self.stride:
            for ss in self.stripe_stats:
                m = WM._Pb()
                for d in ss:
                    m.bytes(1, _stats_msg(d))
                md.bytes(1, bytes(m.b))
            f.bytes(7, _stats_msg(IM.root_stats(total)))
            for i, c in enumerate(self.cols):
                parts = self.all_parts[i]
                f.bytes(7, _stats_msg(IM.column_stats(pa.concat_arrays(parts) if parts else pa.array([], type=c.type))))
            f.u64(8, self.stride)
        f.u64(9, 0xFFFFFFFF)
        ps = WM._Pb()
        ps.u64(1, len(f.b))
        ps.u64(2, 0)
        ps.packed(4, [0, 12])
        ps.u64(5, len(md.b))
        ps.u64(6, 0xFFFFFFFF)
        ps.bytes(8000, b"ORC")
        self.out += md.b + f.b + ps.b + bytes([len(ps.b)])
        return bytes(self.out)


def write_model(batches, schema=None, batch_size=1024, stripe_byte_size=64 << 20, flush_after=(), threshold=0.0, row_index_stride=0, info=None):
    """The file's bytes and its stripes' rows.  info (a dict): gets "dictionary" / "direct", the (string column, stripe) pairs
    written each way, and "decisions", per stripe {column id: dictionary size, or None for a direct column}."""
    schema = schema or batches[0].schema
    if not threshold and not row_index_stride and info is None:
        nested = any(pa.types.is_nested(f.type) for f in schema)
        new = any(NM.TM.is_new(f.type) for f in schema)
        return (NM if nested else (NM.TM if new else WM)).write_model(batches, schema=schema, batch_size=batch_size, stripe_byte_size=stripe_byte_size,
                                                                     flush_after=flush_after)
    m = WriterModel(schema, batch_size, stripe_byte_size, threshold, row_index_stride)
    for i, b in enumerate(batches):
        try:
            m.write(b)
        except ValueError:
            pass
        if i in flush_after:
            m.flush_stripe()
    data = m.close()
    if info is not None:
        info.update({"dictionary": m.n_dictionary, "direct": m.n_direct, "decisions": m.decisions})
    return data, m.stripe_rows()
