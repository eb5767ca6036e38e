"""tests/writer_types_model.py, the yardstick of the writer's Timestamp and Decimal128 columns, checked on the CPU: its files are
read back by pyarrow, every stream is decoded by the oracle's decoders, and its statistics are compared with what pyarrow's own
ORC writer emits for the same values."""
import decimal
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import oracle_lib as O
import writer_types_model as TM
from orcfile import DATA, PRESENT, SECONDARY, OrcFile, pb_fields

def test_nano_code_and_split():
    assert [TM.nano_code(n) for n in (0, 1, 10, 100, 1000, 999_999, 1_000_000, 10 ** 8, 123_456_000, 999_999_999)] == \
        [0, 8, 80, (1 << 3) | 1, (1 << 3) | 2, 999_999 << 3, (1 << 3) | 5, (1 << 3) | 7, (123456 << 3) | 2, 999_999_999 << 3]
    assert TM.ts_split(-1, "ms") == (-1, 999_000_000) and TM.ts_split(-1001, "ms") == (-2, 999_000_000)
    assert TM.ts_stored(-2, 999_000_000) == -1 - TM.TS_BASE and TM.ts_stored(-2, 999_999) == -2 - TM.TS_BASE
    assert TM.ts_stored(TM.TS_BASE, 0) == 0
    for bad in [(-1, 1_000_000), (-1, 999_999_999), (-(1 << 63), 0)]:
        with pytest.raises(ValueError):
            TM.ts_stored(*bad)
    assert TM.ts_stored(-1, 999_999) == -1 - TM.TS_BASE  # (a reader corrects nothing: N <= 999999)


def test_every_timestamp_decodes_by_the_oracle():
    O.lib()
    for v in TM.TS_EDGES_NS + [-(1 << 63), -(1 << 63) + 1]:
        S, N = TM.ts_split(v, "ns")
        st, got = O.decode_timestamp(TM.TS_BASE, TM.ts_stored(S, N), TM.nano_code(N), 3)
        assert st == 0 and got == v, (v, got)


def test_varints_decode_by_the_oracle():
    O.lib()
    vals = TM.dec_edges(38)
    data = b"".join(TM.varint128(v) for v in vals)
    assert max(len(TM.varint128(v)) for v in vals) == 19 and len(TM.varint128(0)) == 1
    st, got = O.varint128(data, len(vals))
    assert st == 0 and got == vals


def test_scale_stream_does_not_depend_on_the_integer_width():
    """the device feeds the scale's encoder i16 values: the bytes are the i64 encoder's"""
    O.lib()
    for s in (0, 1, 2, 17, 38):
        for n in (1, 2, 3, 9, 10, 11, 511, 512, 513, 1030):
            v = np.full(n, s, dtype=np.int64)
            assert O.enc_rle2(v, 2, True) == O.enc_rle2(v, 8, True)


def _streams_decode(data, batches):
    of = OrcFile(data)
    table = pa.Table.from_batches(batches)
    at = 0
    for s in of.stripes:
        if any(t.kind in (9, 18) for t in of.types):
            assert s.writer_timezone == "UTC"
        for ci, f in enumerate(table.schema):
            if not TM.is_new(f.type):
                continue
            arr = table.column(ci).combine_chunks().slice(at, s.number_of_rows)
            n = len(arr) - arr.null_count
            if (ci + 1, PRESENT) in s.streams:
                st, bits = O.boolean(s.streams[(ci + 1, PRESENT)], len(arr))
                assert st == 0 and bits.tolist() == np.asarray(arr.is_valid()).astype(np.uint8).tolist()
            else:
                assert arr.null_count == 0
            if pa.types.is_timestamp(f.type):
                st, a = O.int_rle(s.streams[(ci + 1, DATA)], n, 2, True)
                st2, b = O.int_rle(s.streams[(ci + 1, SECONDARY)], n, 2, False)
                assert st == 0 and st2 == 0
                unit = {"s": 0, "ms": 1, "us": 2, "ns": 3}[f.type.unit]
                got = [O.decode_timestamp(TM.TS_BASE, int(x), int(y), unit)[1] for x, y in zip(a, b)]
                assert got == TM.timestamp_ints(arr)
            else:
                st, got = O.varint128(s.streams[(ci + 1, DATA)], n)
                assert st == 0 and got == TM.decimal_ints(arr)
                st, sc = O.int_rle(s.streams[(ci + 1, SECONDARY)], n, 2, True)
                assert st == 0 and sc.tolist() == [f.type.scale] * n
        at += s.number_of_rows
    assert at == table.num_rows


@pytest.mark.parametrize("batch_size,sbs", [(1, 256), (7, 4096), (1024, 256), (1024, 64 << 20)])
def test_files_read_back(batch_size, sbs):
    O.lib()
    rng = np.random.default_rng(batch_size + sbs)
    n = 300 if batch_size == 1 else 2500
    batches = [TM.mixed_table(n, rng), TM.mixed_table(n // 3, rng, nulls=False)]
    data, rows = TM.write_model(batches, batch_size=batch_size, stripe_byte_size=sbs, flush_after=(0,))
    assert sum(rows) == n + n // 3 and (sbs > 4096 or len(rows) > 2)
    got = po.ORCFile(io.BytesIO(data)).read()
    assert got.equals(TM.read_types(pa.Table.from_batches(batches)))
    _streams_decode(data, batches)


def test_estimate_rule():
    """a Timestamp column counts as two Int64 columns would; a Decimal column its DATA bytes and the scale's encoder"""
    rng = np.random.default_rng(5)
    b = TM.mixed_table(1500, rng)
    t, d = TM.ColumnModel(b.schema.field("tn")), TM.ColumnModel(b.schema.field("d15"))
    t.encode_array(b.column(0))
    d.encode_array(b.column(4))
    import writer_model as WM
    a, c, e = WM.RleV2Model(8, True), WM.RleV2Model(8, False), WM.RleV2Model(8, True)
    for x, y in zip(t.a, t.b):
        a.push(x)
        c.push(y)
    for _ in d.b:
        e.push(2)
    assert t.estimate() == a.estimate() + c.estimate() + 1500 // 8
    assert d.estimate() == len(d.data) + e.estimate() + 1500 // 8


def test_edges_read_back():
    O.lib()
    cols, names = [], []
    for unit in ("s", "ms", "us", "ns"):
        per = TM.NS // TM.UNITS[unit]
        vals = sorted({v // per for v in TM.TS_EDGES_NS if not -TM.NS < v // per * per < 0})
        for tz in (None, "UTC"):
            cols.append(TM.ts_array(vals + [0] * (len(TM.TS_EDGES_NS) - len(vals)), unit, tz))
            names.append("t%s%s" % (unit, tz or ""))
    n = len(TM.TS_EDGES_NS)
    for p, s in ((38, 0), (38, 38), (15, 2), (1, 0)):
        e = TM.dec_edges(p)
        cols.append(TM.dec_array((e * n)[:n], p, s))
        names.append("d%d_%d" % (p, s))
    b = pa.RecordBatch.from_arrays(cols, names=names)
    data, _ = TM.write_model([b, b.slice(3, 9)])
    assert po.ORCFile(io.BytesIO(data)).read().equals(TM.read_types(pa.Table.from_batches([b, b.slice(3, 9)])))
    _streams_decode(data, [b, b.slice(3, 9)])


def test_rejected_batches_change_nothing():
    O.lib()
    good = pa.RecordBatch.from_arrays([TM.ts_array([5, -TM.NS, 7 * TM.NS], "ns")], names=["t"])
    want, _ = TM.write_model([good, good])
    for bad in (-1, -999_000_000):
        b = pa.RecordBatch.from_arrays([TM.ts_array([1, bad, 2], "ns")], names=["t"])
        assert TM.write_model([good, b, good])[0] == want
    for unit, bad in (("ms", -999), ("s", -(1 << 63))):
        g = pa.RecordBatch.from_arrays([TM.ts_array([5, -3000, 7], unit)], names=["t"])
        b = pa.RecordBatch.from_arrays([TM.ts_array([1, bad], unit)], names=["t"])
        assert TM.write_model([g, b, g])[0] == TM.write_model([g, g])[0]


def _pyarrow_stats(table):
    out = io.BytesIO()
    po.write_table(table, out)
    of = OrcFile(out.getvalue())
    return TM.file_statistics(of)[0]


def test_statistics_against_pyarrow_writer():
    """each field pyarrow's ORC writer emits equals the model's (it leaves out nanos at their defaults and the legacy fields).
    Timestamps from 1970 on: for earlier ones pyarrow hands Apache ORC a second rounded toward zero with negative nanoseconds, and
    the statistics it then writes (a millisecond late, a negative nanos field) are not the specification's."""
    O.lib()
    rng = np.random.default_rng(9)
    for seed_shift in (0, 1):
        b = TM.mixed_table(800 + seed_shift, rng, since=0)
        theirs = _pyarrow_stats(pa.Table.from_batches([b]))
        for ci, f in enumerate(b.schema):
            if not TM.is_new(f.type):
                continue
            mine, got = TM.column_stats(b.column(ci)), theirs[ci + 1]
            assert mine["n"] == got["n"] and mine["has_null"] == got["has_null"]
            if pa.types.is_timestamp(f.type):
                assert "timestamp" in got
                for k in range(6):
                    if got["timestamp"][k] is not None:
                        assert got["timestamp"][k] == mine["timestamp"][k], (f.name, k, got, mine)
            else:
                for k in range(3):
                    if got["decimal"][k] is not None:
                        assert decimal.Decimal(got["decimal"][k]) == decimal.Decimal(mine["decimal"][k]), (f.name, k, got, mine)
                        assert mine["decimal"][k] == TM.decimal_string(*_unscaled(got["decimal"][k], f.type.scale)), (f.name, k)


def _unscaled(s, scale):
    with decimal.localcontext() as c:
        c.prec = 80
        return int(decimal.Decimal(s).scaleb(scale)), scale


def test_decimal_strings_and_sum_rule():
    assert [TM.decimal_string(v, s) for v, s in ((0, 2), (5, 2), (-5, 2), (100, 2), (120, 2), (-12345, 2), (7, 0), (1, 38), (-10 ** 37, 38))] == \
        ["0", "0.05", "-0.05", "1", "1.2", "-123.45", "7", "0." + "0" * 37 + "1", "-0.1"]
    top = 10 ** 38 - 1
    inside = TM.column_stats(TM.dec_array([top - 5, 5, -1], 38, 0))
    assert inside["decimal"] == (str(-1), str(top - 5), str(top - 1))
    at = TM.column_stats(TM.dec_array([top, 1], 38, 0))
    assert at["decimal"][2] is None
    wide = TM.column_stats(TM.dec_array([top] * 4 + [-top] * 4 + [3], 38, 0))  # (partial sums pass 2^127, the total does not)
    assert wide["decimal"][2] == "3"


def test_positions_follow_the_streams():
    """a seek to each group's positions decodes that group: run-length streams by (offset, values), DATA of decimals by offset"""
    O.lib()
    rng = np.random.default_rng(11)
    b = TM.mixed_table(1300, rng)
    data, rows = TM.write_model([b])
    s = OrcFile(data).stripes[0]
    for ci in (0, 4):
        arr = b.column(ci)
        pos = TM.model_positions(arr, True, 300)
        valid = np.asarray(arr.is_valid())
        for g, p in enumerate(pos):
            before = int(valid[:g * 300].sum())
            n = int(valid[g * 300:(g + 1) * 300].sum())
            if ci == 0:
                st, got = O.int_rle(s.streams[(1, DATA)][p[3]:], p[4] + n, 2, True)
                want = [TM.ts_stored(*TM.ts_split(v, "ns")) for v in TM.timestamp_ints(arr)][before:before + n]
                assert st == 0 and got[p[4]:].tolist() == want
            else:
                st, got = O.varint128(s.streams[(5, DATA)][p[3]:], n)
                assert st == 0 and got == TM.decimal_ints(arr)[before:before + n]
                st, sc = O.int_rle(s.streams[(5, SECONDARY)][p[4]:], p[5] + n, 2, True)
                assert st == 0 and sc.tolist() == [2] * (p[5] + n)
