"""The row index and statistics the writer adds with a row index stride (orcgpu_writer_set_row_index), restated in Python:
the ColumnStatistics of any range of rows of an Arrow column, and a parser of what a file holds (ROW_INDEX entries, the Metadata
section, Footer.statistics) into the same form.  Statistics are compared as dicts:

    {"n": number_of_values, "has_null": bool, "int": (min, max, sum or None), "double": (min, max, sum), "string": (min, max,
     lower, upper, sum), "binary": sum, "bucket": [true count]}

with only the typed key of the column present, and none when n is 0 (or for floats with a NaN)."""
import bisect
import math
import struct
from fractions import Fraction

import numpy as np
import pyarrow as pa

import writer_model as WM
from orcfile import ROW_INDEX, _packed, pb_fields

I64 = (-(1 << 63), (1 << 63) - 1)
U = Fraction(1, 1 << 53)  # the unit roundoff of f64
ULP0 = 1 << 1074  # every finite f64 is an integer multiple of 2^-1074


def fixed(x):
    """a finite double as an exact integer count of 2^-1074"""
    n, d = x.as_integer_ratio()
    return n << (1074 - (d.bit_length() - 1))


def sum_tol(S, A, n):
    """the bound a float sum is held to (Fractions): 2 (u |S| + gamma_n^2 sum |x|), gamma_n = n u / (1 - n u) -- twice the error
    bound of compensated double-double summation (Ogita, Rump and Oishi, "Accurate sum and dot product", SIAM J. Sci. Comput. 26(6),
    2005, Prop. 4.5); the factor 2 leaves room for the tree and host merges, which Sum2 does not have"""
    g = n * U / (1 - n * U)
    return 2 * (U * abs(S) + g * g * A)


class FloatSum(float):
    """a range's expected double sum R, a float: the exact sum S rounded to nearest (+-inf beyond f64).  For ranges without an
    infinite value it also holds S and sum |x| (`exact`, `abs_sum`: integers in units of 2^-1074) and the number of values n."""

    def __new__(cls, vals):
        pos, neg = any(x == math.inf for x in vals), any(x == -math.inf for x in vals)
        if pos or neg:  # (one sign of infinity: that infinity; both: NaN)
            r = float("nan") if pos and neg else (math.inf if pos else -math.inf)
            self = float.__new__(cls, r)
            self.exact = None
            return self
        S = sum(fixed(x) for x in vals)
        try:
            r = S / ULP0  # (int / int: correctly rounded)
        except OverflowError:
            r = math.inf if S > 0 else -math.inf
        self = float.__new__(cls, r)
        self.exact, self.abs_sum, self.n = S, sum(abs(fixed(x)) for x in vals), len(vals)
        return self

    def S(self):
        return Fraction(self.exact, ULP0)

    def tol(self):
        return sum_tol(self.S(), Fraction(self.abs_sum, ULP0), self.n)

    def admits(self, got):
        """got meets the contract: the same infinity (sign included) for an infinite R; within tol of S for a finite one"""
        if self.exact is None or math.isinf(self):
            return got == self or (math.isnan(got) and math.isnan(self))
        return math.isfinite(got) and abs(Fraction(got) - self.S()) <= self.tol()


def _zz(v):
    return (v >> 1) ^ -(v & 1)


def lower_bound(b):
    cut = 1024
    while cut > 0 and (b[cut] & 0xC0) == 0x80:
        cut -= 1
    return b[:cut]


def upper_bound(b):
    """the lower bound with its last character's code point incremented; trailing U+10FFFF (which has no successor) are dropped
    first; None when nothing is left (then no bound is an upper bound: no StringStatistics)"""
    s = lower_bound(b).decode("utf-8").rstrip("\U0010ffff")
    if not s:
        return None
    cp = ord(s[-1]) + 1
    if 0xD800 <= cp < 0xE000:
        cp = 0xE000
    return (s[:-1] + chr(cp)).encode("utf-8")


def column_stats(arr):
    """arr: a pyarrow Array (the rows of one range)."""
    t = arr.type
    valid = arr.drop_null()
    d = {"n": len(valid), "has_null": arr.null_count > 0}
    if not len(valid):
        return d
    if pa.types.is_integer(t):
        v = [int(x) for x in valid.to_numpy(zero_copy_only=False)]
        s = sum(v)
        d["int"] = (min(v), max(v), s if I64[0] <= s <= I64[1] else None)
    elif pa.types.is_floating(t):
        v = [float(x) for x in valid.to_numpy(zero_copy_only=False).astype(np.float64)]
        if not any(math.isnan(x) for x in v):
            d["double"] = (min(v), max(v), FloatSum(v))  # (min / max: the first of equal values, -0.0 against 0.0)
    elif t in (pa.string(), pa.large_string()):
        v = [x.encode() if isinstance(x, str) else x for x in valid.to_pylist()]
        mn, mx = min(v), max(v)
        up = upper_bound(mx) if len(mx) > 1024 else None
        if len(mx) <= 1024 or up is not None:
            d["string"] = (mn if len(mn) <= 1024 else None, mx if len(mx) <= 1024 else None, lower_bound(mn) if len(mn) > 1024 else None,
                           up, sum(len(x) for x in v))
    elif t in (pa.binary(), pa.large_binary()):
        d["binary"] = sum(len(x) for x in valid.to_pylist())
    elif t == pa.bool_():
        d["bucket"] = [sum(1 for x in valid.to_pylist() if x)]
    return d


def root_stats(rows):
    return {"n": rows, "has_null": False}


def parse_stats(b):
    d = {"n": 0, "has_null": False}
    for f, wt, v in pb_fields(b):
        if f == 1:
            d["n"] = v
        elif f == 10:
            d["has_null"] = bool(v)
        elif f == 2:
            x = {g: _zz(y) for g, _, y in pb_fields(v)}
            d["int"] = (x.get(1), x.get(2), x.get(3))
        elif f == 3:
            x = {g: struct.unpack("<d", bytes(y))[0] for g, _, y in pb_fields(v)}
            d["double"] = (x.get(1), x.get(2), x.get(3))
        elif f == 4:
            x = {g: (bytes(y) if w == 2 else _zz(y)) for g, w, y in pb_fields(v)}
            d["string"] = (x.get(1), x.get(2), x.get(4), x.get(5), x.get(3))
        elif f == 5:
            c = []
            for g, w, y in pb_fields(v):
                c += _packed(y, w)
            d["bucket"] = c
        elif f == 8:
            d["binary"] = {g: _zz(y) for g, _, y in pb_fields(v)}.get(1)
    return d


def same_stats(got, want, rel=1e-9):
    """equal, but for double sums: within rel of the model's, and within FloatSum.tol of the exact sum (an infinite one: equal)"""
    if set(got) != set(want):
        return False
    for k in want:
        if k == "double":
            (a0, a1, a2), (b0, b1, b2) = got[k], want[k]
            if not (a0 == b0 and a1 == b1 and math.copysign(1, a0) == math.copysign(1, b0) and math.copysign(1, a1) == math.copysign(1, b1)):
                return False
            if math.isnan(b2):
                if not math.isnan(a2):
                    return False
            elif math.isinf(b2):
                if a2 != b2:
                    return False
            elif b2 == 0:
                if a2 != b2 and abs(a2 - b2) > 1e-300:
                    return False
            elif not abs(a2 - b2) <= rel * abs(b2):
                return False
            if isinstance(b2, FloatSum) and not b2.admits(a2):
                return False
        elif got[k] != want[k]:
            return False
    return True


def row_index_entries(of, stripe, column):
    """[(positions, stats dict)] of one column's ROW_INDEX stream in one stripe (decompressed)"""
    raw = stripe.streams.get((column, ROW_INDEX), b"")
    b = of._decompress(raw) if of.compression and raw else raw
    out = []
    for f, _, e in pb_fields(b):
        if f != 1:
            continue
        pos, st = [], None
        for g, w, y in pb_fields(e):
            if g == 1:
                pos += _packed(y, w)
            elif g == 2:
                st = parse_stats(y)
        out.append((pos, st))
    return out


def file_statistics(of):
    """(Footer.statistics, [stripe statistics]) of an OrcFile"""
    ps_len = of.buf[-1]
    end = len(of.buf) - 1 - ps_len
    footer = of._decompress(of.buf[end - of.footer_length:end])
    fstats = [parse_stats(v) for f, _, v in pb_fields(footer) if f == 7]
    md_raw = of.buf[end - of.footer_length - of.metadata_length:end - of.footer_length]
    md = of._decompress(md_raw) if of.metadata_length else b""
    sstats = [[parse_stats(c) for g, _, c in pb_fields(v) if g == 1] for f, _, v in pb_fields(md) if f == 1]
    return fstats, sstats


def model_groups(table, stripe_rows, stride):
    """per stripe, per group: [root stats, column stats...]; per stripe: [root, columns]; the file's: [root, columns]"""
    cols = [table.column(i).combine_chunks() for i in range(table.num_columns)]
    groups, stripes, at = [], [], 0
    for rows in stripe_rows:
        g = []
        for r0 in range(0, rows, stride):
            n = min(stride, rows - r0)
            g.append([root_stats(n)] + [column_stats(c.slice(at + r0, n)) for c in cols])
        groups.append(g)
        stripes.append([root_stats(rows)] + [column_stats(c.slice(at, rows)) for c in cols])
        at += rows
    whole = [root_stats(at)] + [column_stats(c) for c in cols]
    return groups, stripes, whole


# ---- positions --------------------------------------------------------------------------------------------------------------
# The runs of a stream as the reference's encoders write them: tests/writer_model.py's state machines, with each run's value
# count recorded (their `runs` hold each run's bytes).  A group's entry in a run-length stream is {byte offset of the run that
# holds its first value, values of that run before it}; past the last value: {the stream's end, 0}.


class Rle2Runs(WM.RleV2Model):
    def __init__(self, int_bytes, signed):
        super().__init__(int_bytes, signed)
        self.counts = []

    def _emit_fixed(self, v, count):
        super()._emit_fixed(v, count)
        self.counts.append(count)

    def _emit_var(self, lits):
        super()._emit_var(lits)
        self.counts.append(len(lits))

    def open_count(self):
        s = self.state
        return 0 if s is None else (1 if s[0] == "one" else (s[2] if s[0] == "fixed" else len(s[1])))


class ByteRuns(WM.ByteRleModel):
    def __init__(self):
        super().__init__()
        self.counts = []

    def _run(self, v, n):
        super()._run(v, n)
        self.counts.append(n)

    def _literals(self, lits):
        super()._literals(lits)
        self.counts.append(len(lits))

    def open_count(self):
        return len(self.lits)


class RunTable:
    """(first value, byte offset) of every run of one stream, and its length"""

    def __init__(self, model, values):
        for v in values:
            model.push(int(v))
        tail = model.finish()
        counts = model.counts + ([model.open_count()] if tail else [])
        sizes = [len(r) for r in model.runs] + ([len(tail)] if tail else [])
        self.starts, self.offsets = [], []
        s = o = 0
        for c, b in zip(counts, sizes):
            self.starts.append(s)
            self.offsets.append(o)
            s += c
            o += b
        self.n, self.total = s, o

    def at(self, x):
        if x >= self.n:
            return self.total, 0
        r = bisect.bisect_right(self.starts, x) - 1
        return self.offsets[r], x - self.starts[r]


def msb_bytes(bits):
    """a bit stream's bytes as the byte encoder sees them: the first bit in the top bit, the spare bits of the last byte 0"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="big").tolist() if len(bits) else []


def chunk_map(raw, block_size):
    """compressed stream -> u -> (offset of the chunk header, bytes into the chunk); the writer's chunks are full blocks but the last"""
    starts, p = [], 0
    while p < len(raw):
        starts.append(p)
        h = raw[p] | (raw[p + 1] << 8) | (raw[p + 2] << 16)
        p += 3 + (h >> 1)

    def f(u):
        k = min(u // block_size, len(starts))
        return (starts[k] if k < len(starts) else len(raw)), u - k * block_size
    return f


def column_streams(arr, has_present):
    """the streams of one column of one stripe as (kind, form, values): form 1 bytes, 2 run-length, 3 bits over byte runs;
    values: what the stream holds (PRESENT / Boolean: bits; strings: DATA the lengths, LENGTH the lengths)"""
    _, _, w = WM.kind_of(arr.type)
    valid = np.asarray(arr.is_valid()).astype(np.uint8) if arr.null_count or arr.buffers()[0] is not None else np.ones(len(arr), np.uint8)
    vv = arr.filter(pa.array(valid.astype(bool)))
    out = []
    if has_present:
        out.append(("PRESENT", 3, valid))
    if w == "rle2":
        out.append(("DATA", 2, vv.to_numpy(zero_copy_only=False).astype(np.int64)))
    elif w == "byte":
        out.append(("DATA", 2, vv.to_numpy(zero_copy_only=False).view(np.uint8)))
    elif w == "float":
        out.append(("DATA", 1, vv.to_numpy(zero_copy_only=False)))
    elif w == "bool":
        out.append(("DATA", 3, vv.to_numpy(zero_copy_only=False).astype(np.uint8)))
    else:
        lens = np.array([len(x.encode() if isinstance(x, str) else x) for x in vv.to_pylist()], dtype=np.int64)
        out.append(("DATA", 1, lens))
        out.append(("LENGTH", 2, lens))
    return w, valid, out


def model_positions(arr, has_present, stride, raws=None, block_size=262144):
    """per group of one column of one stripe: the RowIndexEntry positions.  raws: {kind: compressed stream} of a compressed file"""
    w, valid, streams = column_streams(arr, has_present)
    rows = len(arr)
    before = np.concatenate([[0], np.cumsum(valid)])  # valid values before each row
    per_stream = []
    for kind, form, vals in streams:
        if form == 3:
            table = RunTable(ByteRuns(), msb_bytes(vals))
        elif form == 2 and kind == "LENGTH":
            table = RunTable(Rle2Runs(8 if arr.type in (pa.large_string(), pa.large_binary()) else 4, False), vals)
        elif form == 2 and w == "byte":
            table = RunTable(ByteRuns(), vals)
        elif form == 2:
            table = RunTable(Rle2Runs({pa.int16(): 2, pa.int32(): 4}.get(arr.type, 8), True), vals)
        else:
            table = None
        cum = np.concatenate([[0], np.cumsum(vals)]) if kind == "DATA" and w == "str" else None
        fmap = chunk_map(raws[kind], block_size) if raws is not None else None
        per_stream.append((kind, form, vals, table, cum, fmap))
    out = []
    for r0 in range(0, rows, stride):
        pos = []
        for kind, form, vals, table, cum, fmap in per_stream:
            v = r0 if kind == "PRESENT" else int(before[r0])
            cons = bits = 0
            if form == 3:
                x = v // 8
                if x < (len(vals) + 7) // 8:
                    u, cons = table.at(x)
                    bits = v % 8
                else:
                    u = table.total
            elif form == 2:
                u, cons = table.at(v)
            elif w == "str":
                u = int(cum[v])
            else:
                u = v * vals.dtype.itemsize if arr.type != pa.float32() else v * 4
            pos += list(fmap(u)) if fmap else [u]
            if form >= 2:
                pos.append(cons)
            if form == 3:
                pos.append(bits)
        out.append(pos)
    return out
