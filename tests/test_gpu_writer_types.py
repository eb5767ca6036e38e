"""ArrowWriter's Timestamp and Decimal128 columns on the GPU: the device writer's file is the model's (tests/writer_types_model.py)
byte for byte, and pyarrow and ArrowReaderBuilder read it back equal to the input."""
import ctypes as C
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import gpu_util as G
import oracle_lib as O
import writer_types_model as TM
from orcfile import PRESENT, OrcFile
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder, capi
from orc_rust_amd.capi import OrcGpuError
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from writer_types_model import NS, TS_EDGES_NS, dec_array, dec_edges, mixed_table, ts_array

pytestmark = pytest.mark.gpu

UNSUPPORTED, UNEXPECTED, INVALID_ARGUMENT = 7, 10, 101  # include/orcgpu.h


def gpu_write(batches, schema=None, batch_size=1024, sbs=64 << 20, flush_after=(), comp=None, stride=0):
    out = io.BytesIO()
    b = ArrowWriterBuilder(out, schema or batches[0].schema, ctx=G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(sbs)
    if comp:
        b = b.with_compression(comp, 4096)
    if stride:
        b = b.with_row_index_stride(stride)
    w = b.try_build()
    rejected = []
    for i, x in enumerate(batches):
        try:
            w.write(x)
        except OrcGpuError as e:
            assert e.code == INVALID_ARGUMENT, e
            rejected.append(i)
        if i in flush_after:
            w.flush_stripe()
    w.close()
    rows, stats = w.stripe_rows(), w.stats()
    w.free()
    return out.getvalue(), rows, stats, rejected


def readers(data, batches):
    want = TM.read_types(pa.Table.from_batches(batches))
    assert po.ORCFile(io.BytesIO(data)).read().equals(want), "pyarrow.orc read back something else"
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    assert sum(b.num_rows for b in mine) == want.num_rows
    for i, f in enumerate(want.schema):
        got = pa.concat_arrays([b.column(i) for b in mine])
        assert got.cast(f.type).equals(want.column(i).combine_chunks()), "ArrowReaderBuilder read back something else in %s" % f.name


def check(batches, **kw):
    O.lib()
    want, want_rows = TM.write_model(batches, **{("stripe_byte_size" if k == "sbs" else k): v for k, v in kw.items()})
    got, rows, stats, _ = gpu_write(batches, **kw)
    assert rows == want_rows, (rows, want_rows)
    assert got == want, "file bytes differ from the model's (%d vs %d bytes)" % (len(got), len(want))
    readers(got, batches)
    return rows, stats


def _bitmap(arr):
    bm = pa.py_buffer(np.packbits(np.ones(len(arr), dtype=np.uint8), bitorder="little").tobytes())
    return pa.Array.from_buffers(arr.type, len(arr), [bm] + arr.buffers()[1:], null_count=-1)


@pytest.mark.parametrize("tz", [None, "UTC", "Europe/Paris"])
def test_timestamp_edges(tz):
    cols, names = [], []
    for unit in ("s", "ms", "us", "ns"):
        per = NS // TM.UNITS[unit]
        vals = sorted({v // per for v in TS_EDGES_NS if not -NS < v // per * per < 0}) + [-1001 * (TM.UNITS[unit] // 1000 or 1) - 1, -5]
        vals = [v for v in vals if not -TM.UNITS[unit] < v < 0 or unit == "s"] * 3
        mask = np.arange(len(vals)) % 5 == 1
        cols += [ts_array(vals, unit, tz), _bitmap(ts_array(vals, unit, tz)), ts_array(vals, unit, tz, mask)]
        names += ["p" + unit, "b" + unit, "n" + unit]
    n = min(len(c) for c in cols)
    b = pa.RecordBatch.from_arrays([c.slice(0, n) for c in cols], names=names)
    check([b, b.slice(5, 17)], batch_size=7)


@pytest.mark.parametrize("ps", [(38, 0), (38, 38), (15, 2), (1, 0)])
def test_decimal_edges(ps):
    p, s = ps
    e = dec_edges(p) * 3
    mask = np.arange(len(e)) % 4 == 2
    b = pa.RecordBatch.from_arrays([dec_array(e, p, s), dec_array(e, p, s, mask), dec_array(e, p, s, np.ones(len(e), bool))], names=["d", "n", "allnull"])
    check([b, b.slice(3, len(e) // 2)], batch_size=11)


@pytest.mark.parametrize("n", [65, 257, 4097])
def test_length_scan_crosses_wavefronts_and_blocks(n):
    rng = np.random.default_rng(n)
    mixed = [int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 64)) >> int(rng.integers(0, 120)) for _ in range(n)]
    mixed = [v if i % 3 else -v for i, v in enumerate(mixed)]
    cols, names = [dec_array([v % 10 ** 38 if v >= 0 else -(-v % 10 ** 38) for v in mixed], 38, 0, rng.random(n) < 0.1)], ["mixed"]
    for at in (0, 63, 64, n - 1):
        v = [int(x) for x in rng.integers(-60, 60, n)]
        v[at] = -(10 ** 38 - 1)
        cols.append(dec_array(v, 38, 3))
        names.append("big%d" % at)
    check([pa.RecordBatch.from_arrays(cols, names=names)])


@pytest.mark.parametrize("batch_size", [1, 7, 1024])
@pytest.mark.parametrize("sbs", [256, 4096])
def test_stripe_cuts(batch_size, sbs):
    rng = np.random.default_rng(batch_size * 7 + sbs)
    n = 400 if batch_size == 1 else 2600
    rows, _ = check([mixed_table(n, rng)], batch_size=batch_size, sbs=sbs)
    assert len(rows) > 1


def test_flush_between_writes_and_sticky_present():
    rng = np.random.default_rng(3)
    a, b = mixed_table(700, rng, nulls=False), mixed_table(900, rng)
    rows, _ = check([a, b, a, a], flush_after=(0, 2), batch_size=256, sbs=8192)
    assert len(rows) > 3
    of = OrcFile(gpu_write([a, b, a, a], flush_after=(0, 2), batch_size=256, sbs=8192)[0])
    assert (1, PRESENT) not in of.stripes[0].streams and (1, PRESENT) in of.stripes[-1].streams


def test_round_trips_do_not_grow_with_columns():
    rng = np.random.default_rng(4)
    t = mixed_table(3000, rng)

    def trips(names):
        """per stripe, once the buffers have grown (growing waits for the device, and is counted)"""
        b = pa.RecordBatch.from_arrays([t.column(k) for k in names], names=names)
        w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).try_build()
        w.write(b)
        w.flush_stripe()
        s0 = w.stats()
        for _ in range(3):
            w.write(b)
            w.flush_stripe()
        s1 = w.stats()
        w.close()
        w.free()
        return s1["stripe_round_trips"] - s0["stripe_round_trips"]

    assert trips(["tn"]) == trips(["tn", "tu", "d15", "d38", "d3838", "tm"]) == trips(["d15"]) == trips(["i"]) == 6


@pytest.mark.parametrize("comp", ["snappy", "lz4"])
def test_compressed_streams(comp):
    O.lib()
    rng = np.random.default_rng(6)
    batches = [mixed_table(2500, rng)]
    plain, rows0, _, _ = gpu_write(batches, sbs=16384)
    data, rows, _, _ = gpu_write(batches, sbs=16384, comp=comp)
    assert rows == rows0 and len(rows) > 1
    a, b = OrcFile(plain), OrcFile(data)
    for s0, s1 in zip(a.stripes, b.stripes):
        assert [(k, c) for k, c, _ in s0.stream_list] == [(k, c) for k, c, _ in s1.stream_list]
        for key, raw in s1.streams.items():
            st, out = O.stream_decompress(raw, comp, 4096)
            assert st == 0 and out == bytes(s0.streams[key]), key
    readers(data, batches)


def check_index(data, table, rows, stride):
    O.lib()
    of = OrcFile(data)
    assert of.row_index_stride == stride and [s.number_of_rows for s in of.stripes] == rows
    groups, stripes, whole = TM.model_groups(table, rows, stride)
    cols = [table.column(i).combine_chunks() for i in range(table.num_columns)]
    names = {0: "PRESENT", 1: "DATA", 2: "LENGTH", 5: "SECONDARY"}
    at = 0
    for si, s in enumerate(of.stripes):
        for col in range(1, table.num_columns + 1):
            entries = TM.row_index_entries(of, s, col)
            assert len(entries) == len(groups[si])
            raws = {names[k]: bytes(v) for (c, k), v in s.streams.items() if c == col and k in names} if of.compression else None
            arr = cols[col - 1].slice(at, s.number_of_rows)
            want_pos = TM.model_positions(arr, (col, PRESENT) in s.streams, stride, raws, of.block_size)
            for g, (pos, st) in enumerate(entries):
                assert st == groups[si][g][col], (si, g, col, st, groups[si][g][col])
                assert pos == want_pos[g], (si, g, col, pos, want_pos[g])
        at += s.number_of_rows
    fstats, sstats = TM.file_statistics(of)
    for si, ss in enumerate(sstats):
        for col in range(1, table.num_columns + 1):
            assert ss[col] == stripes[si][col], (si, col, ss[col], stripes[si][col])
    for col in range(1, table.num_columns + 1):
        assert fstats[col] == whole[col], (col, fstats[col], whole[col])


def _index_table(n, rng):
    t = mixed_table(n, rng)
    keep = ["tn", "tu", "ts", "d15", "d38", "d3838"]
    return pa.RecordBatch.from_arrays([t.column(k) for k in keep], names=keep)


@pytest.mark.parametrize("comp", [None, "lz4"])
@pytest.mark.parametrize("stride", [1, 3, 1000])
def test_row_index(stride, comp):
    rng = np.random.default_rng(stride)
    n = 200 if stride < 1000 else 3500
    batches = [_index_table(n, rng), _index_table(n // 2, rng)]
    plain, rows0, _, _ = gpu_write(batches, sbs=8192 if stride < 1000 else 65536, comp=comp)
    data, rows, _, _ = gpu_write(batches, sbs=8192 if stride < 1000 else 65536, comp=comp, stride=stride)
    assert rows == rows0 and len(rows) > 1
    check_index(data, pa.Table.from_batches(batches), rows, stride)
    readers(data, batches)


def _seek(raw, pos, comp, block):
    """the stream from the position's first words on: (the bytes from there, the words left)"""
    if not comp:
        return bytes(raw[pos[0]:]), pos[1:]
    st, out = O.stream_decompress(bytes(raw[pos[0]:]), comp, block)  # (from the chunk header the position names)
    assert st == 0
    return out[pos[1]:], pos[2:]


@pytest.mark.parametrize("comp", [None, "snappy", "lz4"])
@pytest.mark.parametrize("stride", [1, 3, 1000])
def test_seek_to_every_group(stride, comp):
    """a seek to every group by the positions the device writer's ROW_INDEX holds decodes that group: PRESENT, DATA and SECONDARY of
    every Timestamp and Decimal128 column, decompressed from the chunk the position names and decoded by the oracle's decoders"""
    O.lib()
    rng = np.random.default_rng(100 + stride)
    n = 200 if stride < 1000 else 3500
    batches = [_index_table(n, rng), _index_table(n // 2, rng)]
    data, rows, _, _ = gpu_write(batches, sbs=8192 if stride < 1000 else 65536, comp=comp, stride=stride)
    assert len(rows) > 1
    of, table = OrcFile(data), pa.Table.from_batches(batches)
    units = {"s": 0, "ms": 1, "us": 2, "ns": 3}
    at = 0
    for s in of.stripes:
        for col in range(1, table.num_columns + 1):
            arr = table.column(col - 1).combine_chunks().slice(at, s.number_of_rows)
            t = arr.type
            valid = np.asarray(arr.is_valid())
            ints = TM.timestamp_ints(arr) if pa.types.is_timestamp(t) else TM.decimal_ints(arr)
            entries = TM.row_index_entries(of, s, col)
            assert len(entries) == (s.number_of_rows + stride - 1) // stride
            for g, (pos, _) in enumerate(entries):
                r0, r1 = g * stride, min((g + 1) * stride, s.number_of_rows)
                before, k = int(valid[:r0].sum()), int(valid[r0:r1].sum())
                if (col, PRESENT) in s.streams:
                    b, pos = _seek(s.streams[(col, PRESENT)], pos, comp, of.block_size)
                    skip = pos[0] * 8 + pos[1]
                    st, bits = O.boolean(b, skip + r1 - r0)
                    assert st == 0 and bits[skip:].tolist() == valid[r0:r1].astype(np.uint8).tolist(), (col, g)
                    pos = pos[2:]
                else:
                    assert valid.all()
                b, pos = _seek(s.streams[(col, 1)], pos, comp, of.block_size)
                if pa.types.is_timestamp(t):
                    st, secs = O.int_rle(b, pos[0] + k, 2, True)
                    assert st == 0
                    secs, pos = secs[pos[0]:], pos[1:]
                else:
                    st, got = O.varint128(b, k)
                    assert st == 0 and got == ints[before:before + k], (col, g)
                b, pos = _seek(s.streams[(col, 5)], pos, comp, of.block_size)
                st, sec2 = O.int_rle(b, pos[0] + k, 2, not pa.types.is_timestamp(t))
                assert st == 0 and len(pos) == 1
                sec2 = sec2[pos[0]:]
                if pa.types.is_timestamp(t):
                    got = [O.decode_timestamp(TM.TS_BASE, int(x), int(y), units[t.unit])[1] for x, y in zip(secs, sec2)]
                    assert got == ints[before:before + k], (col, g)
                else:
                    assert sec2.tolist() == [t.scale] * k, (col, g)
        at += s.number_of_rows


def test_decimal_sum_boundary():
    top = 10 ** 38 - 1
    cases = [[top - 5, 5, -1], [top, 1], [top] * 4 + [-top] * 4 + [3], [-top, -1]]
    n = max(len(c) for c in cases)
    b = pa.RecordBatch.from_arrays([dec_array(c + [0] * (n - len(c)), 38, 0) for c in cases], names=["inside", "at", "wide", "neg"])
    data, rows, _, _ = gpu_write([b], stride=1000)
    check_index(data, pa.Table.from_batches([b]), rows, 1000)
    st = TM.file_statistics(OrcFile(data))[0]
    assert st[1]["decimal"][2] == str(top - 1) and st[2]["decimal"][2] is None and st[3]["decimal"][2] == "3" and st[4]["decimal"][2] is None


def test_sorted_files_prune():
    """the reader's row group filter takes a timestamp bound as milliseconds (Int64) and compares decimals as strings: values of
    equal digit counts, so that the strings' order is the numbers'"""
    n, stride = 4000, 500
    ts = ts_array([1_600_000_000 * NS + i * 1_000_000_007 for i in range(n)], "ns")
    dec = dec_array([(1000 + i) * 100 for i in range(n)], 15, 2)
    b = pa.RecordBatch.from_arrays([ts, dec], names=["t", "d"])
    data, rows, _, _ = gpu_write([b], stride=stride)
    groups, _, _ = TM.model_groups(pa.Table.from_batches([b]), rows, stride)
    assert rows == [n]
    cut_ms = 1_600_000_000_000 + 2_600_000
    want_t = sum(stride for g in groups[0] if g[1]["timestamp"][3] >= cut_ms)
    got = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).with_predicate(P.gte("t", V.Int64(cut_ms))).build())
    assert sum(x.num_rows for x in got) == want_t and 0 < want_t < n
    want_d = sum(stride for g in groups[0] if g[2]["decimal"][1] >= "3100")
    got = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).with_predicate(P.gte("d", V.Utf8("3100"))).build())
    assert sum(x.num_rows for x in got) == want_d and 0 < want_d < n


def test_rejections():
    O.lib()
    for unit, good, bads in (("ns", [5, -NS, 7 * NS], [-1, -999_000_000]), ("ms", [5, -3000, 7], [-999]), ("s", [5, -3, 7], [-(1 << 63)])):
        plain = pa.RecordBatch.from_arrays([ts_array(good, unit)], names=["t"])
        want, _ = TM.write_model([plain, plain])
        for bad in bads:
            b = pa.RecordBatch.from_arrays([ts_array([1, bad, 2], unit, None, np.array([True, False, False]))], names=["t"])
            got, _, _, rejected = gpu_write([plain, b, plain])
            assert rejected == [1] and got == want
            # the same value in a null slot is no value: the batch is taken, and reads back equal
            ok = pa.RecordBatch.from_arrays([ts_array([1, bad, 2], unit, None, np.array([False, True, False]))], names=["t"])
            check([plain, ok, plain])
    for t in (pa.decimal256(40, 2), pa.decimal128(10, -1), pa.list_(pa.decimal128(10, 2)), pa.date32()):
        with pytest.raises(OrcGpuError) as e:
            ArrowWriterBuilder(io.BytesIO(), pa.schema([("x", t)]), ctx=G.ctx()).try_build()
        assert e.value.code == UNSUPPORTED
    w = ArrowWriterBuilder(io.BytesIO(), pa.schema([("x", pa.decimal128(10, 2))]), ctx=G.ctx()).try_build()
    for t in (pa.decimal128(11, 2), pa.decimal128(10, 3)):
        with pytest.raises(OrcGpuError) as e:
            w.write(pa.RecordBatch.from_arrays([dec_array([1], t.precision, t.scale)], names=["x"]))
        assert e.value.code == UNEXPECTED
    w.free()


class _ArrowArray(C.Structure):
    pass


_ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64), ("n_children", C.c_int64),
                        ("buffers", C.POINTER(C.c_void_p)), ("children", C.POINTER(C.POINTER(_ArrowArray))), ("dictionary", C.c_void_p),
                        ("release", C.c_void_p), ("private_data", C.c_void_p)]


@pytest.mark.parametrize("name,column,t", [("decimal.orc", 1, pa.decimal128(10, 5)), ("pyarrow_timestamps.orc", 1, pa.timestamp("ns")),
                                           ("pyarrow_timestamps.orc", 2, pa.timestamp("ns", "UTC"))])
def test_device_resident_input(name, column, t):
    """a decode's output handed to the writer from its device buffers (ORCGPU_ENC_ON_DEVICE): the bytes of the same rows from the
    host, which read back equal"""
    import os
    O.lib()
    of = OrcFile(os.path.join(os.path.dirname(__file__), "golden", "data", name))
    s, ot = of.stripes[0], of.types[column]
    cols = [{"column_id": column, "orc_type": ot.kind, "encoding": s.encodings[column][0], "precision": ot.precision, "scale": ot.scale}]
    streams = [(c, k, bytes(v)) for (c, k), v in s.streams.items() if c == column and k != 6]
    res = G.gpu_decode(s.number_of_rows, cols, streams, ts_base=TM.TS_BASE)
    assert res.status()[0] == 0
    v, host = res.view(0, 0), res.batch(0, 0)
    m = v.length
    elem = 16 if pa.types.is_decimal(t) else 8
    assert v.values_bytes == m * elem
    bufs = [pa.py_buffer(host["validity"]) if host["validity"] is not None else None, pa.py_buffer(host["values"])]
    hb = pa.RecordBatch.from_arrays([pa.Array.from_buffers(t, m, bufs, null_count=-1)], names=["x"])
    want, want_rows = TM.write_model([hb], batch_size=1000, stripe_byte_size=2048)
    child = _ArrowArray()
    cbufs = (C.c_void_p * 2)(v.validity, v.values)
    child.length, child.null_count, child.offset, child.n_buffers, child.n_children, child.buffers = m, v.null_count, 0, 2, 0, cbufs
    root = _ArrowArray()
    rbufs = (C.c_void_p * 1)(None)
    kids = (C.POINTER(_ArrowArray) * 1)(C.pointer(child))
    root.length, root.null_count, root.offset, root.n_buffers, root.n_children, root.buffers, root.children = m, 0, 0, 1, 1, rbufs, kids
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, hb.schema, ctx=G.ctx()).with_batch_size(1000).with_stripe_byte_size(2048).try_build()
    sbuf = (C.c_uint8 * 72)()
    hb.schema._export_to_c(C.addressof(sbuf))
    try:
        w.write_c(C.addressof(sbuf), C.addressof(root), capi.ENC_ON_DEVICE)
    finally:
        rel = C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0]
        rel(C.addressof(sbuf))
    w.close()
    assert w.stripe_rows() == want_rows
    w.free()
    res.free()
    assert out.getvalue() == want
    readers(want, [hb])


def test_large():
    rng = np.random.default_rng(300000)
    n = 300000
    ns = np.cumsum(rng.integers(0, 3 * NS, n)) + 1_500_000_000 * NS
    ns[::5] = ns[::5] // 1000 * 1000
    b = pa.RecordBatch.from_arrays(
        [ts_array(ns, "ns", None, rng.random(n) < 0.05), dec_array(rng.integers(-10 ** 9, 10 ** 9, n).tolist(), 15, 2),
         dec_array([int(x) << 60 for x in rng.integers(-10 ** 12, 10 ** 12, n)], 38, 4, rng.random(n) < 0.5)], names=["t", "money", "wide"])
    rows, _ = check([b], sbs=1 << 20)
    assert len(rows) > 1
