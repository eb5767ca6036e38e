"""Timestamp and Decimal128 columns of the writer, restated in Python over tests/writer_model.py's RleV2Model / WriterModel: the
bytes of the file, the stripe cut, the statistics and the row index positions.

Timestamp(unit, tz): a valid value v splits into S = floor(v / units_per_second) and N, the rest in nanoseconds.  DATA is signed
RLE v2 of S' - 1420070400, with S' = S + 1 when S < 0 and N > 999999 (ORC-763: a reader takes such a stored second for one
earlier); SECONDARY is unsigned RLE v2 of the nanosecond code.  S == -1 with N > 999999 and a stored second outside i64 have no
encoding: ValueError.  Decimal128(p, s): DATA is the values as zigzag varints, not run-length encoded; SECONDARY is signed RLE v2
of s, once per valid value.  Both: DATA, SECONDARY, [PRESENT], DIRECT_V2.

The estimate that cuts stripes: a Timestamp column counts its two encoders' estimates, a Decimal column the DATA bytes so far and
the scale encoder's estimate; PRESENT as for every column.  Every stripe footer of a file with a Timestamp column carries
writer_timezone = "UTC"."""
import decimal
import os

import numpy as np
import pyarrow as pa

import index_model as IM
import oracle_lib as O
import writer_model as WM
from orcfile import pb_fields

TS_BASE = 1420070400
UNITS = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}
I64 = (-(1 << 63), (1 << 63) - 1)

# pyarrow's ORC reader looks the writer's zone ("UTC") up in the tz database and fails without one.  On a host without
# /usr/share/zoneinfo, and with TZDIR unset, importing this module points TZDIR at the tzdata package's copy for the whole process,
# as orc_rust_amd.capi.load() does for the library; with neither, the read-back checks fail with pyarrow's own message.
if not os.path.isdir("/usr/share/zoneinfo") and "TZDIR" not in os.environ:
    try:
        import tzdata
        os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
    except ImportError:
        pass


def is_new(t):
    return pa.types.is_timestamp(t) or pa.types.is_decimal128(t)


def kind_of(t):
    """(ORC Type.Kind, ColumnEncoding.Kind, column writer)"""
    if pa.types.is_timestamp(t):
        return (18 if t.tz else 9), 2, "ts"
    if pa.types.is_decimal128(t):
        if not (1 <= t.precision <= 38 and 0 <= t.scale <= t.precision):
            raise NotImplementedError("unsupported datatype %s" % t)
        return 14, 2, "dec"
    return WM.kind_of(t)


def ts_split(v, unit):
    ups = UNITS[unit]
    S = v // ups
    return S, (v - S * ups) * (10 ** 9 // ups)


def ts_stored(S, N):
    """the DATA stream's value"""
    if S == -1 and N > 999999:
        raise ValueError("a timestamp within the second before 1970 has no encoding")
    st = (S + 1 if S < 0 and N > 999999 else S) - TS_BASE
    if not I64[0] <= st <= I64[1]:
        raise ValueError("a timestamp's second is too far from 2015")
    return st


def nano_code(N):
    if N == 0:
        return 0
    z, m = 0, N
    while m % 10 == 0:
        m //= 10
        z += 1
    return (m << 3) | (z - 1) if z >= 2 else N << 3


def varint128(v):
    z = ((v << 1) ^ (v >> 127)) & ((1 << 128) - 1)
    out = bytearray()
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)
    return bytes(out)


def decimal_ints(arr):
    """the unscaled integers of a Decimal128 array's valid values"""
    scale = arr.type.scale
    out = []
    for d in arr.drop_null().to_pylist():
        sign, digits, exp = d.as_tuple()
        m = int("".join(map(str, digits)) or "0")
        m = m * 10 ** (exp + scale) if exp + scale >= 0 else m // 10 ** -(exp + scale)
        out.append(-m if sign else m)
    return out


def timestamp_ints(arr):
    return [int(x) for x in arr.drop_null().cast(pa.int64()).to_numpy(zero_copy_only=False)]


def read_types(table):
    """the types the file reads back as: TIMESTAMP as Timestamp(ns), TIMESTAMP_INSTANT as Timestamp(ns, UTC); the others as
    writer_model's files do"""
    fields = []
    for f in table.schema:
        t = f.type
        if pa.types.is_timestamp(t):
            t = pa.timestamp("ns", "UTC" if t.tz else None)
        t = {pa.large_string(): pa.string(), pa.large_binary(): pa.binary()}.get(t, t)
        fields.append(pa.field(f.name, t))
    return table.cast(pa.schema(fields))


def decimal_string(v, scale):
    """minimal form: a '-' sign, no exponent, trailing fractional zeros and a bare point removed, '0' for zero"""
    s = str(abs(v)).rjust(scale + 1, "0")
    if scale:
        s = (s[:-scale] + "." + s[-scale:]).rstrip("0").rstrip(".")
    return ("-" if v < 0 else "") + s


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------
NS = 10 ** 9
TS_EDGES_NS = [0, 1, 10, 100, 1000, 999_999, 1_000_000, 10 ** 8, 123_456_000, 999_999_999, -NS, -NS - 1, -999_999_000 - NS,
               TS_BASE * NS, TS_BASE * NS + 5, (1 << 63) - 1, -(1 << 63) + 854775808, 2 * NS + 120, -5 * NS + 1200]
# (1677-09-21 00:12:44 exactly: the first second pyarrow's reader takes -- it multiplies the second by 10^9 before adding the
# nanoseconds; the oracle's decoder also takes the values below it)


def ts_array(vals, unit, tz=None, mask=None):
    return pa.array(np.array(vals, dtype=np.int64), type=pa.int64(), mask=mask).cast(pa.timestamp(unit, tz))


def dec_array(ints, p, s, mask=None):
    with decimal.localcontext() as c:
        c.prec = 60
        vals = [decimal.Decimal(v).scaleb(-s) for v in ints]
    if mask is not None:
        vals = [None if m else v for v, m in zip(vals, mask)]
    return pa.array(vals, type=pa.decimal128(p, s))


def dec_edges(p):
    e = [0, 1, -1, 63, 64, -64, -65]
    for k in range(1, 19):
        e += [(1 << (7 * k - 1)) - 1, 1 << (7 * k - 1), -(1 << (7 * k - 1)), -(1 << (7 * k - 1)) - 1]
    e += [10 ** 38 - 1, -(10 ** 38 - 1)]
    return [v for v in e if abs(v) < 10 ** p]


def mixed_table(n, rng, nulls=True, since=-3 * 10 ** 18):
    """four Timestamp columns (every unit, with and without a zone), four Decimal128 columns, an Int64 and a Utf8 column"""
    ns = rng.integers(since, 3 * 10 ** 18, n)
    ns[(ns > -NS) & (ns < 0)] = 0
    ns[::7] = ns[::7] // NS * NS
    ns[::11] = ns[::11] // 1000 * 1000
    ns[n // 2: n // 2 + 40] = 1_600_000_000 * NS
    money = rng.integers(-10 ** 9, 10 ** 9, n).tolist()
    big = [int(x) * 10 ** 19 + int(y) for x, y in zip(rng.integers(-10 ** 18, 10 ** 18, n), rng.integers(0, 10 ** 18, n))]
    m = (lambda: rng.random(n) < 0.2) if nulls else (lambda: None)
    return pa.RecordBatch.from_arrays(
        [ts_array(ns, "ns", None, m()), ts_array(ns // 1000, "us", "UTC", m()), ts_array(ns // 10 ** 6, "ms"), ts_array(ns // NS, "s", "Europe/Paris", m()),
         dec_array(money, 15, 2, m()), dec_array(big, 38, 0, m()), dec_array(rng.integers(-9, 10, n).tolist(), 1, 0), dec_array(big, 38, 38, m()),
         pa.array(rng.integers(-100, 100, n)), pa.array(["s%d" % (i % 13) for i in range(n)], mask=m())],
        names=["tn", "tu", "tm", "ts", "d15", "d38", "d1", "d3838", "i", "u"])


class ColumnModel:
    """a Timestamp or Decimal128 column's stripe encoder, with WM.ColumnModel's interface"""

    def __init__(self, field):
        self.orc_kind, self.encoding, self.w = kind_of(field.type)
        self.type = field.type
        self.present = None
        self.reset()

    def reset(self):
        self.a, self.b, self.data, self.n_present = [], [], bytearray(), 0
        self.enc_a = WM.RleV2Model(8, True) if self.w == "ts" else None
        self.enc_b = WM.RleV2Model(8, self.w == "dec")
        if self.present is not None:
            self.present = []

    def encode_array(self, arr):
        has_bitmap = arr.buffers()[0] is not None
        valid = np.ones(len(arr), dtype=bool) if not has_bitmap else np.asarray(arr.is_valid())
        if has_bitmap and self.present is None:
            self.present = [1] * self.n_present
        if self.present is not None:
            self.present.extend(valid.astype(np.uint8).tolist())
        self.n_present += len(arr)
        if self.w == "ts":
            for v in timestamp_ints(arr):
                S, N = ts_split(v, self.type.unit)
                st, code = ts_stored(S, N), nano_code(N)
                self.a.append(st)
                self.b.append(code)
                self.enc_a.push(st)
                self.enc_b.push(code)
        else:
            for v in decimal_ints(arr):
                self.data += varint128(v)
                self.b.append(self.type.scale)
                self.enc_b.push(self.type.scale)

    def estimate(self):
        e = self.enc_b.estimate() + (self.enc_a.estimate() if self.w == "ts" else len(self.data))
        if self.present is not None:
            e += len(self.present) // 8
        return e

    def finish(self):
        """[(kind, bytes)]: DATA, SECONDARY, [PRESENT]"""
        b = np.array(self.b, dtype=np.int64)
        sec = O.enc_rle2(b, 8, self.w == "dec") if len(b) else b""
        assert b"".join(self.enc_b.runs) + self.enc_b.finish() == sec
        if self.w == "ts":
            a = np.array(self.a, dtype=np.int64)
            data = O.enc_rle2(a, 8, True) if len(a) else b""
            assert b"".join(self.enc_a.runs) + self.enc_a.finish() == data
        else:
            data = bytes(self.data)
        out = [(1, data), (5, sec)]
        if self.present is not None:
            p = np.array(self.present, dtype=np.uint8)
            out.append((0, O.enc_boolean(np.packbits(p, bitorder="little"), len(p)) if len(p) else b""))
        return out


class WriterModel(WM.WriterModel):
    def __init__(self, schema, batch_size=1024, stripe_byte_size=64 << 20):
        self.schema, self.bs, self.sbs = schema, batch_size, stripe_byte_size
        self.cols = [ColumnModel(f) if is_new(f.type) else WM.ColumnModel(f) for f in schema]
        self.out = bytearray(b"ORC")
        self.stripes = []
        self.rows = 0
        self.has_ts = any(pa.types.is_timestamp(f.type) for f in schema)

    def write(self, batch):
        """a batch with a value that has no encoding changes nothing (ValueError)"""
        for f, arr in zip(self.schema, batch.columns):
            if pa.types.is_timestamp(f.type):
                for v in timestamp_ints(arr):
                    ts_stored(*ts_split(v, f.type.unit))
        super().write(batch)

    def flush_stripe(self):
        start = len(self.out)
        streams, data_len = [], 0
        for i, c in enumerate(self.cols):
            for kind, b in c.finish():
                self.out += b
                data_len += len(b)
                streams.append((kind, i + 1, len(b)))
        f = WM._Pb()
        for kind, col, ln in streams:
            m = WM._Pb()
            m.u64(1, kind)
            m.u64(2, col)
            m.u64(3, ln)
            f.bytes(1, bytes(m.b))
        for enc in [0] + [c.encoding for c in self.cols]:
            m = WM._Pb()
            m.u64(1, enc)
            f.bytes(2, bytes(m.b))
        if self.has_ts:
            f.bytes(3, b"UTC")
        self.out += f.b
        self.stripes.append((start, data_len, len(f.b), self.rows))
        self.rows = 0
        for c in self.cols:
            c.reset()

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
        root.packed(2, list(range(1, len(self.cols) + 1)))
        for fd in self.schema:
            root.bytes(3, fd.name.encode())
        f.bytes(4, bytes(root.b))
        for c in self.cols:
            t = WM._Pb()
            t.u64(1, c.orc_kind)
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
    """as WM.write_model; a batch without an encoding is skipped, as the writer rejects it"""
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


# ---- statistics -------------------------------------------------------------------------------------------------------------
# {"timestamp": (min ms, max ms, min ms UTC, max ms UTC, min nanos + 1, max nanos + 1)}: floor milliseconds, the nanoseconds within
# the millisecond plus one; absent when a bound's milliseconds leave i64.  {"decimal": (min, max, sum or None)}: strings at the
# column's scale; the sum when |sum| < 10^38.


def column_stats(arr):
    t = arr.type
    if not is_new(t):
        return IM.column_stats(arr)
    valid = arr.drop_null()
    d = {"n": len(valid), "has_null": arr.null_count > 0}
    if not len(valid):
        return d
    if pa.types.is_timestamp(t):
        sn = [ts_split(v, t.unit) for v in timestamp_ints(arr)]
        (s0, n0), (s1, n1) = min(sn), max(sn)
        lo, hi = s0 * 1000 + n0 // 10 ** 6, s1 * 1000 + n1 // 10 ** 6
        if I64[0] <= lo and hi <= I64[1]:
            d["timestamp"] = (lo, hi, lo, hi, n0 % 10 ** 6 + 1, n1 % 10 ** 6 + 1)
    else:
        v = decimal_ints(arr)
        s = sum(v)
        d["decimal"] = (decimal_string(min(v), t.scale), decimal_string(max(v), t.scale), decimal_string(s, t.scale) if abs(s) < 10 ** 38 else None)
    return d


def parse_stats(b):
    d = IM.parse_stats(b)
    for f, _, v in pb_fields(b):
        if f == 6:
            x = {g: bytes(y).decode() for g, _, y in pb_fields(v)}
            d["decimal"] = (x.get(1), x.get(2), x.get(3))
        elif f == 9:
            x = {g: y for g, _, y in pb_fields(v)}
            d["timestamp"] = tuple(IM._zz(x[g]) if g in x else None for g in (1, 2, 3, 4)) + (x.get(5), x.get(6))
    return d


def model_groups(table, stripe_rows, stride):
    """as IM.model_groups, with the new types' statistics"""
    cols = [table.column(i).combine_chunks() for i in range(table.num_columns)]
    groups, stripes, at = [], [], 0
    for rows in stripe_rows:
        g = []
        for r0 in range(0, rows, stride):
            n = min(stride, rows - r0)
            g.append([IM.root_stats(n)] + [column_stats(c.slice(at + r0, n)) for c in cols])
        groups.append(g)
        stripes.append([IM.root_stats(rows)] + [column_stats(c.slice(at, rows)) for c in cols])
        at += rows
    return groups, stripes, [IM.root_stats(at)] + [column_stats(c) for c in cols]


def row_index_entries(of, stripe, column):
    raw = stripe.streams.get((column, 6), b"")
    b = of._decompress(raw) if of.compression and raw else raw
    out = []
    for f, _, e in pb_fields(b):
        if f == 1:
            pos, st = [], None
            for g, w, y in pb_fields(e):
                if g == 1:
                    pos += IM._packed(y, w)
                elif g == 2:
                    st = parse_stats(y)
            out.append((pos, st))
    return out


def file_statistics(of):
    ps_len = of.buf[-1]
    end = len(of.buf) - 1 - ps_len
    footer = of._decompress(of.buf[end - of.footer_length:end])
    fstats = [parse_stats(v) for f, _, v in pb_fields(footer) if f == 7]
    md_raw = of.buf[end - of.footer_length - of.metadata_length:end - of.footer_length]
    md = of._decompress(md_raw) if of.metadata_length else b""
    return fstats, [[parse_stats(c) for g, _, c in pb_fields(v) if g == 1] for f, _, v in pb_fields(md) if f == 1]


# ---- positions --------------------------------------------------------------------------------------------------------------
# Timestamp: PRESENT, DATA and SECONDARY as run-length streams.  Decimal: PRESENT, DATA as a byte stream, SECONDARY run-length.


def model_positions(arr, has_present, stride, raws=None, block_size=262144):
    """per group of one column of one stripe: the RowIndexEntry positions; raws: {"PRESENT" / "DATA" / "SECONDARY": compressed stream}"""
    t = arr.type
    if not is_new(t):
        return IM.model_positions(arr, has_present, stride, raws, block_size)
    valid = np.asarray(arr.is_valid()).astype(np.uint8)
    before = np.concatenate([[0], np.cumsum(valid)])
    streams = []
    if has_present:
        streams.append(("PRESENT", IM.RunTable(IM.ByteRuns(), IM.msb_bytes(valid)), None))
    if pa.types.is_timestamp(t):
        sn = [ts_split(v, t.unit) for v in timestamp_ints(arr)]
        streams.append(("DATA", IM.RunTable(IM.Rle2Runs(8, True), [ts_stored(S, N) for S, N in sn]), None))
        streams.append(("SECONDARY", IM.RunTable(IM.Rle2Runs(8, False), [nano_code(N) for _, N in sn]), None))
    else:
        lens = [len(varint128(v)) for v in decimal_ints(arr)]
        streams.append(("DATA", None, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)))
        streams.append(("SECONDARY", IM.RunTable(IM.Rle2Runs(8, True), [t.scale] * len(lens)), None))
    out = []
    for r0 in range(0, len(arr), stride):
        pos = []
        for kind, table, cum in streams:
            fmap = IM.chunk_map(raws[kind], block_size) if raws is not None else None
            v = r0 if kind == "PRESENT" else int(before[r0])
            tail = []
            if kind == "PRESENT":
                x = v // 8
                if x < (len(valid) + 7) // 8:
                    u, cons = table.at(x)
                    tail = [cons, v % 8]
                else:
                    u, tail = table.total, [0, 0]
            elif table is not None:
                u, cons = table.at(v)
                tail = [cons]
            else:
                u = int(cum[v])
            pos += (list(fmap(u)) if fmap else [u]) + tail
        out.append(pos)
    return out
