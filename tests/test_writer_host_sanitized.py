"""The ArrowWriter's device-free host code under AddressSanitizer + UBSan on the CPU: tests/hostcheck/writer_host_check.cpp compiles
orc_rust_amd/csrc/orcgpu_writer_host.inc -- the text liborcgpu.so is built from -- into a stand-alone program; its answers are
judged by tests/index_model.py, Python's decimal and tables written out here.  No GPU, nothing loaded into Python."""
import decimal
import math
import os
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import index_model as IM
import stats_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g1", "-O0"]
UNSUPPORTED, INVALID = 7, 101


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("writer_host") / "writer_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "writer_host_check.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-3000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines) + 1 and got[-1].startswith("built 3 "), got[-3:]
        return got[:-1]
    return run


def unhex(s):
    return b"" if s == "-" else bytes.fromhex(s)


def test_string_bounds(ask):
    tail = "x" * 8
    longs = []
    for ch in ("a", "é", "€", "\U0001f600"):              # a 1 024-byte prefix ending in a 1/2/3/4-byte character
        longs.append(("p" * (1024 - len(ch.encode())) + ch + tail).encode())
    longs.append(("p" * 1022 + "€" + tail).encode())             # the cut falls inside a character
    longs.append(("p" * 1020 + "\U0010ffff" + tail).encode())         # ends in U+10FFFF once
    longs.append(("\U0010ffff" * 256 + tail).encode())                # ... all the way down: no upper bound
    longs.append(("p" * 1021 + "퟿" + tail).encode("utf-8", "surrogatepass"))  # the successor would be a surrogate
    for c in SC.string_cases():
        for v in c.get("values", []):
            b = v.encode() if isinstance(v, str) else v
            if len(b) > 1024:
                longs.append(b)
    got = ask(["lower " + b[:1025].hex() for b in longs] + ["upper " + b[:1025].hex() for b in longs])
    for i, b in enumerate(longs):
        assert unhex(got[i]) == IM.lower_bound(b), i
        up = IM.upper_bound(b)
        assert (got[len(longs) + i] == "none") if up is None else (unhex(got[len(longs) + i]) == up), i
    assert got[len(longs) + 6] == "none"


def _minimal(v, scale):
    d = decimal.Decimal(v).scaleb(-scale)
    s = format(d, "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return "0" if s in ("-0", "") else s


def test_decimal_strings(ask):
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        vals = [0, 1, -1, -(1 << 127), 10 ** 38 - 1, -(10 ** 38 - 1)] + [s * 10 ** k for k in (1, 2, 3, 17, 37, 38) for s in (1, -1)] + [1234500, -70]
        points = [(v, sc) for v in vals for sc in (0, 1, 2, 38)]
        got = ask(["dec %d %d %d" % ((v >> 64) & (2 ** 64 - 1), v & (2 ** 64 - 1), sc) for v, sc in points])
        for (v, sc), g in zip(points, got):
            assert g == _minimal(v, sc), (v, sc, g)


NV = 12           # values of a group; four groups a column
BIG = 2.0 ** 960  # device/col_stats.hip: IX_BIG -- values from here on are summed apart, scaled by 2^-64


def _bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def _dd(vals):
    """the exact sum of a few doubles as a double-double"""
    hi = math.fsum(vals)
    return hi, math.fsum(vals + [-hi])


def _column(case):
    """the case's values spread over 4 NV fillers, as stats_cases.column_values spreads them over its larger groups"""
    f = case["filler"]
    v = list(f(NV)) if callable(f) else [f] * (4 * NV)
    k = len(case["values"])
    for i, x in enumerate(case["values"]):
        v[i * 4 * NV // k] = x
    return v


def _float_record(g, has_null):
    """a group's record as ix_stats_kernel leaves it (device/writer_kinds.h: IxRec): NaNs apart, the first of equal values the
    minimum / maximum, two double-double sums split at 2^960"""
    v = [x for x in g if not math.isnan(x)]
    mn = mx = 0.0
    for i, x in enumerate(v):
        if i == 0 or x < mn:
            mn = x
        if i == 0 or x > mx:
            mx = x
    hi, lo = _dd([x for x in v if abs(x) < BIG])
    big = [x for x in v if abs(x) >= BIG]
    if any(math.isinf(x) for x in big):
        bhi, blo = sum(x for x in big if math.isinf(x)), 0.0  # (one sign: that infinity; both: NaN)
    else:
        bhi, blo = _dd([x * 2.0 ** -64 for x in big])
    return "%d %s %d %d" % (len(g), " ".join(_bits(x) for x in (mn, mx, hi, lo, bhi, blo)), len(v) < len(g), has_null)


def _int_record(g, has_null):
    s = sum(g)
    return "%d %d %d %d %d %d" % (len(g), min(g, default=0), max(g, default=0), s >> 64, s & (2 ** 64 - 1), has_null)


def test_statistics_merge_and_messages(ask):
    """per-group records in, the merged ColumnStatistics out: stats_cases.py's float-sum (the scaled accumulator's, the overflowing
    and the infinite ones included), float min/max, int64 and small-int cases, and a NaN; every second column with nulls"""
    columns = []  # (command, Arrow format, pyarrow type, values with None for nulls)
    for np_t, fmt, typ in ((np.float64, "g", pa.float64()), (np.float32, "f", pa.float32())):
        cases = SC.float_sum_cases(np_t)[0] + SC.float_minmax_cases(np_t) + [{"name": "nan", "values": [1.0, float("nan"), 2.0], "filler": 0.5}]
        columns += [("dbl", fmt, typ, [float(x) for x in _column(c)]) for c in cases]
    columns += [("int", "l", pa.int64(), [int(x) for x in _column(c)]) for c in SC.int64_cases()]
    fmts = {pa.int8(): "c", pa.int16(): "s", pa.int32(): "i"}
    for name, arr in SC.small_int_table(NV, np.random.default_rng(5)).items():
        columns.append(("int", fmts[arr.type], arr.type, arr.to_pylist()))
    lines, wants = [], []
    for k, (cmd, fmt, typ, vals) in enumerate(columns):
        groups = [vals[g * NV:(g + 1) * NV] for g in range(4)]
        if k % 2 and None not in vals:
            groups[1] = groups[1] + [None]
        recs = [(_float_record if cmd == "dbl" else _int_record)([x for x in g if x is not None], None in g) for g in groups]
        lines.append("%s %s %d %s" % (cmd, fmt, len(recs), " ".join(recs)))
        wants.append(IM.column_stats(pa.array([x for g in groups for x in g], type=typ)))
    assert len(lines) > 40 and any(w["has_null"] for w in wants) and any("double" not in w and "int" not in w for w in wants)
    for ln, g, want in zip(lines, ask(lines), wants):
        assert IM.same_stats(IM.parse_stats(unhex(g)), want), (ln[:60], IM.parse_stats(unhex(g)), want)


def _md(pairs):
    b = struct.pack("<i", len(pairs))
    for k, v in pairs:
        b += struct.pack("<i", len(k)) + k + struct.pack("<i", len(v)) + v
    return b


def test_metadata_blobs_round_trip(ask):
    blobs = [_md([]), _md([(b"k", b"v")]), _md([(b"", b""), (b"key" * 50, bytes(range(256)))])]
    got = ask(["meta " + (b + b"\xff\xff").hex() for b in blobs])  # (what follows the blob is not part of it)
    assert [unhex(g) for g in got] == blobs


# (ORC Type.Kind, ColumnEncoding.Kind, parent, child index), preorder, of writer_host_check.cpp's schema
BOOLEAN, BYTE, SHORT, INT, LONG, FLOAT, DOUBLE, STRING, BINARY, TIMESTAMP, LIST, MAP, STRUCT, DECIMAL, INSTANT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 18
DIRECT, DIRECT_V2 = 0, 2
TREE = [(BOOLEAN, DIRECT, -1, 0), (BYTE, DIRECT, -1, 1), (SHORT, DIRECT_V2, -1, 2), (INT, DIRECT_V2, -1, 3), (LONG, DIRECT_V2, -1, 4),
        (FLOAT, DIRECT, -1, 5), (DOUBLE, DIRECT, -1, 6), (STRING, DIRECT_V2, -1, 7), (STRING, DIRECT_V2, -1, 8), (BINARY, DIRECT_V2, -1, 9),
        (BINARY, DIRECT_V2, -1, 10), (TIMESTAMP, DIRECT_V2, -1, 11), (INSTANT, DIRECT_V2, -1, 12), (DECIMAL, DIRECT_V2, -1, 13),
        (MAP, DIRECT_V2, -1, 14), (STRING, DIRECT_V2, 14, 0), (STRUCT, DIRECT, 14, 1), (LIST, DIRECT_V2, 16, 0), (INT, DIRECT_V2, 17, 0),
        (DOUBLE, DIRECT, 16, 1), (LIST, DIRECT_V2, -1, 15), (LONG, DIRECT_V2, 20, 0)]


def test_schema_walk_and_refusals(ask):
    names = ["fixed_size_list", "dictionary", "decimal_below_list", "d:39,2", "d:5,6", "d:10,2,256", "map_without_entries"]
    got = ask(["tree"] + ["refuse " + n for n in names])
    t = got[0].split()
    assert t[:3] == ["0", str(len(TREE)), "1"]
    assert [tuple(int(x) for x in c.split(",")) for c in t[3:]] == TREE
    assert [int(g) for g in got[1:]] == [UNSUPPORTED] * 6 + [INVALID]


# A column's streams, (Stream.Kind, encoder, signed, bytes of a value), from the ORC specification v1, "Column Encodings" (Boolean:
# bits over byte RLE; tinyint: byte RLE; smallint / int / bigint: signed Integer RLE v2; float / double: IEEE bytes; string and
# binary DIRECT_V2: DATA bytes + unsigned LENGTH; string DICTIONARY_V2: unsigned DATA ids, unsigned LENGTH, DICTIONARY_DATA bytes;
# timestamp: signed DATA seconds + unsigned SECONDARY; decimal: DATA varints + signed SECONDARY scale; struct: PRESENT alone; list /
# map: unsigned LENGTH), in the order the reference's stripe writer emits a column's streams (writer/stripe.rs:128-150 with
# writer/column.rs:147-157, :240-250, :371-383: the value streams, PRESENT last)
PRESENT, DATA, LENGTH, DICTIONARY_DATA, SECONDARY = 0, 1, 2, 3, 5
RLE2, BYTE_RLE, BITS, COPY = 0, 1, 2, 3
STREAMS = {
    (0, 8, 0): [(DATA, RLE2, 1, 8)], (0, 2, 0): [(DATA, RLE2, 1, 2)], (1, 1, 0): [(DATA, BYTE_RLE, 0, 1)], (2, 4, 0): [(DATA, COPY, 0, 0)],
    (3, 1, 0): [(DATA, BITS, 0, 1)], (4, 4, 0): [(DATA, COPY, 0, 0), (LENGTH, RLE2, 0, 4)], (4, 8, 0): [(DATA, COPY, 0, 0), (LENGTH, RLE2, 0, 8)],
    (4, 4, 1): [(DATA, RLE2, 0, 4), (LENGTH, RLE2, 0, 4), (DICTIONARY_DATA, COPY, 0, 0)],
    (5, 8, 0): [(DATA, RLE2, 1, 8), (SECONDARY, RLE2, 0, 8)], (6, 16, 0): [(DATA, COPY, 0, 0), (SECONDARY, RLE2, 1, 2)],
    (7, 0, 0): [], (8, 4, 0): [(LENGTH, RLE2, 0, 4)], (8, 8, 0): [(LENGTH, RLE2, 0, 8)],
}


def test_stream_description(ask):
    keys = [(k, present) for k in STREAMS for present in (0, 1)]
    got = ask(["streams %d %d %d %d 1" % (k[0], k[1], present, k[2]) for k, present in keys])
    for (k, present), g in zip(keys, got):
        f = g.split()
        want = STREAMS[k] + ([(PRESENT, BITS, 0, 1)] if present else [])
        assert int(f[0]) == len(STREAMS[k]), (k, g)
        assert [tuple(int(x) for x in s.split(",")[:4]) for s in f[1:]] == want, (k, present, g)
    # without a row index nothing has positions
    f = ask(["streams 4 4 1 0 0"])[0].split()
    assert all(s.split(",")[4] == "-1" for s in f[1:])
