"""A restatement of the reference's ArrowWriter (src/arrow_writer.rs:34-262, src/writer/stripe.rs, src/writer/column.rs) in Python,
over the oracle's pinned encoders (oracle_lib.enc_rle2 / enc_byte_rle / enc_boolean): the bytes of the file it writes.

The stripe cut needs the encoders' EstimateMemory after every slice: restated here value by value -- the two greedy state machines
(RleV2Encoder::process_value, rle_v2/mod.rs:284-360; ByteRleEncoder::process_value, byte.rs:47-114) with the bytes of each run
they write out (the oracle's encoding of the run alone).  `self_check` asserts that those runs, strung together with what finish()
writes, are the oracle's whole-stream bytes."""
import numpy as np
import pyarrow as pa

import oracle_lib as O

# Arrow type -> (ORC Type.Kind, ColumnEncoding.Kind, column writer)
_KINDS = [
    (pa.bool_(), 0, 0, "bool"), (pa.int8(), 1, 0, "byte"), (pa.int16(), 2, 2, "rle2"), (pa.int32(), 3, 2, "rle2"),
    (pa.int64(), 4, 2, "rle2"), (pa.float32(), 5, 0, "float"), (pa.float64(), 6, 0, "float"), (pa.string(), 7, 2, "str"),
    (pa.large_string(), 7, 2, "str"), (pa.binary(), 8, 2, "str"), (pa.large_binary(), 8, 2, "str"),
]


def kind_of(t):
    for at, orc, enc, w in _KINDS:
        if t == at:
            return orc, enc, w
    raise NotImplementedError("unsupported datatype %s" % t)


class RleV2Model:
    """RleV2Encoder<N, S>: the state machine; `emitted` = data.len()."""

    def __init__(self, int_bytes, signed):
        self.ib, self.signed = int_bytes, signed
        self.state, self.emitted, self.runs = None, 0, []

    def _emit_fixed(self, v, count):
        b = O.enc_rle2(np.full(count, v, dtype=np.int64), self.ib, self.signed)
        self.runs.append(b)
        self.emitted += len(b)

    def _emit_var(self, lits):
        b = O.enc_rle2_variable_run(np.array(lits, dtype=np.int64), self.ib, self.signed)
        self.runs.append(b)
        self.emitted += len(b)

    def push(self, v):
        s = self.state
        if s is None:
            self.state = ("one", v)
        elif s[0] == "one":
            self.state = ("fixed", v, 2) if v == s[1] else ("var", [s[1], v])
        elif s[0] == "fixed":
            _, fv, cnt = s
            if v == fv:
                cnt += 1
                if cnt == 512:
                    self._emit_fixed(fv, cnt)
                    self.state = None
                else:
                    self.state = ("fixed", fv, cnt)
            elif cnt == 2:
                self.state = ("var", [fv, fv, v])
            else:
                self._emit_fixed(fv, cnt)
                self.state = ("one", v)
        else:
            lits = s[1]
            if len(lits) >= 2 and v == lits[-1] and v == lits[-2]:
                del lits[-2:]
                self._emit_var(lits)
                self.state = ("fixed", v, 3)
            else:
                lits.append(v)
                if len(lits) == 512:
                    self._emit_var(lits)
                    self.state = None

    def estimate(self):
        return self.emitted

    def finish(self):
        """take_inner's flush (rle_v2/mod.rs:364-390): the bytes of the open run"""
        s = self.state
        if s is None:
            return b""
        if s[0] == "one":
            return O.enc_rle2(np.array([s[1]], dtype=np.int64), self.ib, self.signed)
        if s[0] == "fixed":
            return O.enc_rle2(np.full(s[2], s[1], dtype=np.int64), self.ib, self.signed)
        return O.enc_rle2_variable_run(np.array(s[1], dtype=np.int64), self.ib, self.signed)


class ByteRleModel:
    """ByteRleEncoder: the state machine; estimate = writer.len() + num_literals."""

    def __init__(self):
        self.lits, self.tail, self.run_value, self.emitted = [], 0, None, 0
        self.runs = []  # the bytes of every run written out (write_run / write_literals, byte.rs:176-197)

    def _run(self, v, n):
        self.runs.append(bytes([n - 3, v]))
        self.emitted += 2

    def _literals(self, lits):
        self.runs.append(bytes([(256 - len(lits)) & 0xFF]) + bytes(lits))
        self.emitted += 1 + len(lits)

    def push(self, v):
        if not self.lits:
            self.run_value, self.lits, self.tail = None, [v], 1
        elif self.run_value is not None:
            if v == self.run_value:
                self.lits.append(v)
                if len(self.lits) == 130:
                    self._run(self.run_value, 130)
                    self.lits, self.tail, self.run_value = [], 0, None
            else:
                self._run(self.run_value, len(self.lits))
                self.run_value, self.lits, self.tail = None, [v], 1
        else:
            self.tail = self.tail + 1 if v == self.lits[-1] else 1
            if self.tail == 3:
                if len(self.lits) + 1 == 3:
                    self.run_value = v
                    self.lits.append(v)
                else:
                    self._literals(self.lits[: len(self.lits) - 2])
                    self.run_value, self.lits = v, [v, v, v]
            else:
                self.lits.append(v)
                if len(self.lits) == 128:
                    self._literals(self.lits)
                    self.lits, self.tail, self.run_value = [], 0, None

    def estimate(self):
        return self.emitted + len(self.lits)

    def finish(self):
        if not self.lits:
            return b""
        return bytes([len(self.lits) - 3, self.run_value]) if self.run_value is not None else bytes([(256 - len(self.lits)) & 0xFF]) + bytes(self.lits)


class ColumnModel:
    def __init__(self, field):
        self.orc_kind, self.encoding, self.w = kind_of(field.type)
        self.type = field.type
        self.ib = {pa.int16(): 2, pa.int32(): 4, pa.int64(): 8}.get(field.type, 0)
        self.ob = 8 if field.type in (pa.large_string(), pa.large_binary()) else 4
        self.fw = 4 if field.type == pa.float32() else 8
        self.present = None  # list of 0 / 1 once a validity buffer arrived
        self.reset()

    def reset(self):
        self.vals, self.strs, self.n_present = [], [], 0
        self.enc = RleV2Model(self.ib, True) if self.w == "rle2" else (ByteRleModel() if self.w == "byte" else None)
        if self.w == "str":
            self.enc = RleV2Model(self.ob, False)
        if self.present is not None:
            self.present = []

    def encode_array(self, arr):
        if self.w == "str" and len(arr) == 0:
            return
        has_bitmap = arr.buffers()[0] is not None
        valid = np.ones(len(arr), dtype=bool) if not has_bitmap else np.asarray(arr.is_valid())
        if has_bitmap and self.present is None:
            self.present = [1] * self.n_present  # back-filled (column.rs:116-121)
        if self.present is not None:
            self.present.extend(valid.astype(np.uint8).tolist())
        self.n_present += len(arr)
        vv = arr.filter(pa.array(valid)) if has_bitmap else arr
        if self.w == "str":
            items = [x.as_py() for x in vv]
            items = [x.encode() if isinstance(x, str) else x for x in items]
            self.strs.extend(items)
            for b in items:
                self.enc.push(len(b))
        else:
            v = vv.to_numpy(zero_copy_only=False)
            if self.w == "bool":
                v = v.astype(np.uint8)
            self.vals.append(v)
            if self.enc is not None:
                for x in (v.view(np.uint8) if self.w == "byte" else v.astype(np.int64)).tolist():
                    self.enc.push(x)

    def n_valid(self):
        return sum(len(v) for v in self.vals) if self.w != "str" else len(self.strs)

    def estimate(self):
        e = 0
        if self.w in ("rle2", "byte"):
            e = self.enc.estimate()
        elif self.w == "float":
            e = self.fw * self.n_valid()
        elif self.w == "bool":
            e = self.n_valid() // 8
        else:
            e = sum(len(s) for s in self.strs) + self.enc.estimate()
        if self.present is not None:
            e += len(self.present) // 8
        return e

    def finish(self):
        """[(kind, bytes)]: DATA, [LENGTH], [PRESENT]"""
        out = []
        if self.w == "str":
            out.append((1, b"".join(self.strs)))
            lens = np.array([len(s) for s in self.strs], dtype=np.int64)
            data = O.enc_rle2(lens, self.ob, False) if len(lens) else b""
            out.append((2, data))
            self._self_check(data)
        else:
            v = np.concatenate(self.vals) if self.vals else np.zeros(0)
            if self.w == "rle2":
                data = O.enc_rle2(v.astype(np.int64), self.ib, True) if len(v) else b""
                self._self_check(data)
            elif self.w == "byte":
                data = O.enc_byte_rle(v.astype(np.int8)) if len(v) else b""
                self._self_check(data)
            elif self.w == "float":
                data = np.ascontiguousarray(v.astype(np.float32 if self.fw == 4 else np.float64)).tobytes()
            else:
                data = O.enc_boolean(np.packbits(v.astype(np.uint8), bitorder="little"), len(v)) if len(v) else b""
            out.append((1, data))
        if self.present is not None:
            p = np.array(self.present, dtype=np.uint8)
            out.append((0, O.enc_boolean(np.packbits(p, bitorder="little"), len(p)) if len(p) else b""))
        return out

    def _self_check(self, whole):
        # the runs written out during the stripe, then what finish() writes, are the oracle's whole stream
        assert b"".join(self.enc.runs) + self.enc.finish() == whole, "runs of the state machine differ from the oracle's stream"


class _Pb:
    def __init__(self):
        self.b = bytearray()

    def varint(self, v):
        while v >= 0x80:
            self.b.append((v & 0x7F) | 0x80)
            v >>= 7
        self.b.append(v)

    def u64(self, f, v):
        self.varint(f << 3)
        self.varint(v)

    def bytes(self, f, data):
        self.varint((f << 3) | 2)
        self.varint(len(data))
        self.b += data

    def packed(self, f, vals):
        if vals:
            m = _Pb()
            for v in vals:
                m.varint(v)
            self.bytes(f, bytes(m.b))


class WriterModel:
    """ArrowWriterBuilder::new(..).with_batch_size(..).with_stripe_byte_size(..).try_build() and what follows."""

    def __init__(self, schema, batch_size=1024, stripe_byte_size=64 << 20):
        self.schema, self.bs, self.sbs = schema, batch_size, stripe_byte_size
        self.cols = [ColumnModel(f) for f in schema]
        self.out = bytearray(b"ORC")
        self.stripes = []  # (offset, data_length, footer_length, rows)
        self.rows = 0

    def estimate(self):
        return sum(c.estimate() for c in self.cols)

    def write(self, batch):
        if not batch.schema.equals(self.schema, check_metadata=True):
            raise ValueError("RecordBatch doesn't match expected schema")
        n = batch.num_rows
        for off in range(0, n, self.bs):
            sl = batch.slice(off, min(self.bs, n - off))
            for c, arr in zip(self.cols, sl.columns):
                c.encode_array(arr)
            self.rows += sl.num_rows
            if self.estimate() > self.sbs:
                self.flush_stripe()

    def flush_stripe(self):
        start = len(self.out)
        streams, data_len = [], 0
        for i, c in enumerate(self.cols):
            for kind, b in c.finish():
                self.out += b
                data_len += len(b)
                streams.append((kind, i + 1, len(b)))
        f = _Pb()
        for kind, col, ln in streams:
            m = _Pb()
            m.u64(1, kind)
            m.u64(2, col)
            m.u64(3, ln)
            f.bytes(1, bytes(m.b))
        for enc in [0] + [c.encoding for c in self.cols]:
            m = _Pb()
            m.u64(1, enc)
            f.bytes(2, bytes(m.b))
        self.out += f.b
        self.stripes.append((start, data_len, len(f.b), self.rows))
        self.rows = 0
        for c in self.cols:
            c.reset()

    def close(self):
        if self.rows > 0:
            self.flush_stripe()
        f = _Pb()
        f.u64(1, 3)
        f.u64(2, sum(s[1] + s[2] for s in self.stripes) + 3)
        for off, dl, fl, rows in self.stripes:
            m = _Pb()
            for k, v in enumerate((off, 0, dl, fl, rows)):
                m.u64(k + 1, v)
            f.bytes(3, bytes(m.b))
        root = _Pb()
        root.u64(1, 12)
        root.packed(2, list(range(1, len(self.cols) + 1)))
        for fd in self.schema:
            root.bytes(3, fd.name.encode())
        f.bytes(4, bytes(root.b))
        for c in self.cols:
            t = _Pb()
            t.u64(1, c.orc_kind)
            f.bytes(4, bytes(t.b))
        f.u64(6, sum(s[3] for s in self.stripes))
        f.u64(9, 0xFFFFFFFF)
        ps = _Pb()
        ps.u64(1, len(f.b))
        ps.u64(2, 0)
        ps.packed(4, [0, 12])
        ps.u64(5, 0)
        ps.u64(6, 0xFFFFFFFF)
        ps.bytes(8000, b"ORC")
        self.out += f.b + ps.b + bytes([len(ps.b)])
        return bytes(self.out)

    def stripe_rows(self):
        return [s[3] for s in self.stripes]


def write_model(batches, schema=None, batch_size=1024, stripe_byte_size=64 << 20, flush_after=()):
    """The file's bytes and its stripes' row counts; flush_after: indexes of batches after whose write flush_stripe() is called."""
    m = WriterModel(schema or batches[0].schema, batch_size, stripe_byte_size)
    for i, b in enumerate(batches):
        m.write(b)
        if i in flush_after:
            m.flush_stripe()
    data = m.close()
    return data, m.stripe_rows()
