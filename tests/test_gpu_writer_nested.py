"""ArrowWriter's Struct, List and Map columns on the GPU: the device writer's file is the model's (tests/writer_nested_model.py)
byte for byte, and pyarrow.orc and ArrowReaderBuilder read it back equal to the input.  Shapes are chosen by where the
flattening kernels can go wrong (wavefront and RLE-run limits, both row paths, slicing at every level), not by workload."""
import ctypes as C
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import arrow_util as A
import gpu_util as G
import oracle_lib as O
import writer_model as WM
import writer_nested_model as NM
import writer_types_model as TM
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder, capi
from orc_rust_amd.capi import OrcGpuError
from test_gpu_writer_compression import check_chunked
from writer_nested_model import expected_paths, ints, list_array, map_array, raw_list, strings

pytestmark = pytest.mark.gpu

UNSUPPORTED, UNEXPECTED, INVALID_ARGUMENT = 7, 10, 101  # include/orcgpu.h


def gpu_write(batches, schema=None, batch_size=1024, sbs=64 << 20, flush_after=(), comp=None, block=4096):
    out = io.BytesIO()
    b = ArrowWriterBuilder(out, schema or batches[0].schema, ctx=G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(sbs)
    if comp:
        b = b.with_compression(comp, block)
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
    want = NM.read_types(pa.Table.from_batches(batches))
    assert po.ORCFile(io.BytesIO(data)).read().equals(want), "pyarrow.orc read back something else"
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    assert sum(b.num_rows for b in mine) == want.num_rows
    for i, f in enumerate(want.schema):
        got = pa.concat_arrays([b.column(i) for b in mine]) if mine else pa.array([], type=f.type)
        assert got.to_pylist() == want.column(i).to_pylist(), "ArrowReaderBuilder read back something else in %s" % f.name


def check(batches, **kw):
    O.lib()
    want, want_rows = NM.write_model(batches, **{("stripe_byte_size" if k == "sbs" else k): v for k, v in kw.items()})
    got, rows, stats, _ = gpu_write(batches, **kw)
    assert rows == want_rows, (rows, want_rows)
    assert got == want, "file bytes differ from the model's (%d vs %d bytes)" % (len(got), len(want))
    readers(got, [b for b in batches])
    return rows, stats


def struct_array(n, rng, nulls=0.2):
    kids = [pa.array(rng.integers(-5, 5, n).astype(np.int64)),                       # no validity buffer: never a PRESENT stream
            pa.array(rng.integers(0, 1 << 40, n), mask=rng.random(n) < 0.3),
            strings(rng, 0.2)(n), pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.1)]
    return pa.StructArray.from_arrays(kids, names=["plain", "n", "s", "b"], mask=pa.array(rng.random(n) < nulls) if nulls else None)


def mixed(n, rng):
    return pa.RecordBatch.from_arrays(
        [list_array(n, rng, ints(rng, np.int32, 0.1), nulls=0.2),                       # null lists own ranges: the gather
         list_array(n, rng, lambda m: pa.array(rng.random(m).astype(np.float32))),      # no nulls: a slice
         struct_array(n, rng), list_array(n, rng, strings(rng, 0.2), nulls=0.1),
         pa.array(np.arange(n, dtype=np.int32))], names=["lg", "lf", "st", "ls", "i"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 1025])
def test_row_counts_at_wavefront_and_run_limits(n):
    rng = np.random.default_rng(n)
    b = mixed(n, rng)
    _, stats = check([b], batch_size=64)
    if n >= 63:
        assert stats["nested_gathers"] > 0 and stats["nested_slices"] > 0, stats
    # child counts on the same edges: lists of exactly one element each under a null-free parent, and of eight
    for k in (1, 8):
        offs = np.arange(n + 1, dtype=np.int32) * k
        one = pa.ListArray.from_arrays(pa.array(offs), pa.array(rng.integers(0, 3, n * k).astype(np.int16)))
        check([pa.RecordBatch.from_arrays([one], names=["l"])], batch_size=100)


def test_fast_path_and_gather_path_are_told_apart():
    child = pa.array(np.arange(9, dtype=np.int32))
    offs = pa.array([0, 2, 5, 5, 9], type=pa.int32())

    def with_nulls(nulls):
        bm = np.ones(4, dtype=bool)
        bm[list(nulls)] = False
        return pa.Array.from_buffers(pa.list_(pa.int32()), 4, [pa.py_buffer(np.packbits(bm, bitorder="little").tobytes()), offs.buffers()[1]], children=[child])
    for nulls in ((), (2,), (0,), (3,), (1,), (0, 3), (0, 1, 3), (1, 3), (1, 2)):
        # rows 0, 1 and 3 own ranges, row 2 is empty: null, it leaves one contiguous range and nothing is gathered
        b = pa.RecordBatch.from_arrays([with_nulls(nulls)], names=["l"])
        _, stats = check([b])
        want = (0, 0) if set(nulls) >= {0, 1, 3} else ((1, 0) if set(nulls) & {0, 1, 3} else (0, 1))
        assert (stats["nested_gathers"], stats["nested_slices"]) == want == expected_paths(b.column(0)), (nulls, stats)
    # first, last and in the middle of a longer column; all of them null
    rng = np.random.default_rng(1)
    for at in ([0, 1], [198, 199], [100], list(range(200))):
        a = list_array(200, rng, ints(rng, np.int32), empties=0.0, max_len=3)
        bm = np.ones(200, dtype=bool)
        bm[at] = False
        a = pa.Array.from_buffers(a.type, 200, [pa.py_buffer(np.packbits(bm, bitorder="little").tobytes()), a.buffers()[1]], children=[a.values])
        _, stats = check([pa.RecordBatch.from_arrays([a], names=["l"])])
        assert (stats["nested_gathers"], stats["nested_slices"]) == expected_paths(a), (at, stats)
        assert expected_paths(a)[0] == (len(at) < 200 and bool(np.diff(np.asarray(a.offsets))[at].sum()))
    # a null Struct above drops rows too
    s = pa.StructArray.from_arrays([pa.array(np.arange(50))], names=["x"], mask=pa.array(np.arange(50) % 7 == 3))
    _, stats = check([pa.RecordBatch.from_arrays([s], names=["s"])])
    assert stats["nested_gathers"] == 1


def test_empty_lists_and_all_empty_columns():
    rng = np.random.default_rng(4)
    e = list_array(130, rng, ints(rng, np.int64), empties=1.0)
    en = list_array(130, rng, strings(rng), nulls=0.3, empties=1.0)
    some = list_array(130, rng, ints(rng, np.int8, 0.2), nulls=0.2, empties=0.7)
    check([pa.RecordBatch.from_arrays([e, en, some], names=["e", "en", "some"])], batch_size=16)


def test_null_structs_over_null_and_non_null_children():
    rng = np.random.default_rng(6)
    n = 300
    inner = struct_array(n, rng, 0.3)
    outer = pa.StructArray.from_arrays([inner, pa.array(rng.random(n)), TM.dec_array([int(v) for v in rng.integers(-99999, 99999, n)], 12, 4, rng.random(n) < 0.2)],
                                       names=["in", "f", "d"], mask=pa.array(rng.random(n) < 0.3))
    never_null = struct_array(n, rng, 0)
    all_null = pa.StructArray.from_arrays([pa.array(np.arange(n))], names=["x"], mask=pa.array(np.ones(n, dtype=bool)))
    b = pa.RecordBatch.from_arrays([outer, never_null, all_null], names=["o", "nn", "an"])
    check([b, b.slice(11, 200)], batch_size=37)


def test_slices_at_every_level_and_int64_offsets():
    rng = np.random.default_rng(8)
    n = 260
    for large in (False, True):
        for nulls in (0.0, 0.25):
            big = list_array(n + 10, rng, ints(rng, np.int32, 0.1), nulls=nulls, large=large, empties=0.1)
            # the child array sliced (its offset != 0), the offsets rebased onto it; then the list array itself sliced
            shift = int(np.asarray(big.offsets)[5])
            offs = (np.asarray(big.offsets)[5:] - shift).astype(np.int64 if large else np.int32)
            bm = np.asarray(big.is_valid())[5:]
            bufs = [pa.py_buffer(np.packbits(bm, bitorder="little").tobytes()) if nulls else None, pa.py_buffer(offs.tobytes())]
            a = pa.Array.from_buffers(big.type, n + 5, bufs, children=[big.values.slice(shift)]).slice(3, n)
            assert a.offset == 3 and a.values.offset == shift and np.asarray(a.offsets)[0] != 0
            bools = list_array(n + 5, rng, lambda m: pa.array(rng.random(m + 3) < 0.5, mask=rng.random(m + 3) < 0.2).slice(3), nulls=nulls, large=large).slice(3, n)
            st = pa.StructArray.from_arrays([a.slice(1), bools.slice(1), strings(rng, 0.1)(n + 6).slice(7)], names=["l", "b", "s"],
                                            mask=pa.array(rng.random(n - 1) < nulls) if nulls else None).slice(2, n - 4)
            b = pa.RecordBatch.from_arrays([a.slice(4, n - 4), bools.slice(4, n - 4), st], names=["l", "b", "st"])
            check([b, b.slice(9, 100)], batch_size=50)


def test_strings_binaries_timestamps_and_maps_under_lists():
    rng = np.random.default_rng(10)
    n = 200
    for nulls in (0.0, 0.2):
        ls = list_array(n, rng, strings(rng, 0.2), nulls=nulls)
        lb = list_array(n, rng, strings(rng, 0.2, binary=True), nulls=nulls)
        empties = list_array(n, rng, lambda m: pa.array([""] * m), nulls=nulls)
        lt = list_array(n, rng, lambda m: TM.ts_array([int(v) for v in rng.integers(0, 1 << 50, m)], "us", "UTC", rng.random(m) < 0.1), nulls=nulls)
        lls = list_array(n, rng, lambda m: pa.array(["x" * int(v) for v in rng.integers(0, 9, m)], type=pa.large_string()), nulls=nulls, large=True)
        keys = list_array(n, rng, strings(rng), nulls=nulls)
        m = map_array(keys, pa.array(rng.integers(0, 99, len(keys.values)), mask=rng.random(len(keys.values)) < 0.2))
        b = pa.RecordBatch.from_arrays([ls, lb, empties, lt, lls, m], names=["ls", "lb", "e", "lt", "lls", "m"])
        _, stats = check([b, b.slice(13, 150)], batch_size=64)
        assert (stats["nested_gathers"] > 0) == (nulls > 0)


def test_depth_three_and_present_from_the_second_batch():
    rng = np.random.default_rng(12)

    def deep(n, nulls):
        def structs(m):
            kids = [list_array(m, rng, ints(rng, np.int32, nulls), nulls=nulls), strings(rng, nulls)(m)]
            return pa.StructArray.from_arrays(kids, names=["a", "s"], mask=pa.array(rng.random(m) < nulls) if nulls else None)
        return pa.RecordBatch.from_arrays([list_array(n, rng, structs, nulls=nulls)], names=["l"])
    plain, nulls = deep(150, 0.0), deep(150, 0.2)
    assert plain.schema == nulls.schema
    # no column has a PRESENT stream until the second batch: back-filled at every level; then a stripe where all have one
    check([plain, nulls, plain], batch_size=32)
    check([plain, nulls, plain], flush_after=(0, 1))


@pytest.mark.parametrize("batch_size", [1, 7])
def test_stripe_cuts_between_long_lists(batch_size):
    rng = np.random.default_rng(13)
    a = list_array(120, rng, ints(rng, np.int32), nulls=0.2, max_len=60)
    m = list_array(120, rng, lambda k: pa.array(rng.random(k)), max_len=30)
    b = pa.RecordBatch.from_arrays([a, m, struct_array(120, rng)], names=["l", "m", "s"])
    rows, _ = check([b, b.slice(5, 60), b], batch_size=batch_size, sbs=1500, flush_after=(1,))
    assert len(rows) > 5
    rows, _ = check([b], batch_size=batch_size, sbs=1)  # (a slice of empty lists alone estimates 0 bytes and is not cut off)
    assert len(rows) > 60 // batch_size
    # zero-row stripes
    w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).try_build()
    w.flush_stripe()
    w.write(b)
    w.flush_stripe()
    w.flush_stripe()
    w.close()
    assert w.stripe_rows() == [0, 120, 0]
    w.free()


@pytest.mark.parametrize("codec", ["snappy", "lz4"])
@pytest.mark.parametrize("block", [64, 262144])
def test_compressed_streams_are_the_uncompressed_files(codec, block):
    rng = np.random.default_rng(15)
    b = mixed(400, rng)
    plain, rows0, _, _ = gpu_write([b, b.slice(3, 300)], batch_size=64, sbs=4000)
    got, rows, _, _ = gpu_write([b, b.slice(3, 300)], batch_size=64, sbs=4000, comp=codec, block=block)
    assert rows == rows0 and len(rows) > 2
    check_chunked(got, plain, codec, block)
    readers(got, [b, b.slice(3, 300)])


def test_bad_offsets_reject_the_batch_and_the_writer_stays_usable():
    O.lib()
    rng = np.random.default_rng(16)
    child = pa.array(np.arange(10, dtype=np.int32))
    n = 70
    down = np.minimum(np.arange(n + 1) // 8, 10)
    down[40] = 2                                     # descends in the middle
    far = np.minimum(np.arange(n + 1) // 8, 10)
    far[33] = 1 << 30                                # far past the child, then back: a kernel must not follow it
    for large in (False, True):  # (int32 and int64 offsets: each against a writer of its own schema)
        good = pa.RecordBatch.from_arrays([list_array(100, rng, ints(rng, np.int32), nulls=0.2, large=large)], names=["l"])
        want, _ = NM.write_model([good, good, good])
        for offs in ([0, 4, 2, 6], [0, 100, 6, 9], down, far):
            b = pa.RecordBatch.from_arrays([raw_list(offs, child, large=large)], names=["l"])
            assert b.schema == good.schema
            got, _, _, rejected = gpu_write([good, b, good, b, good])
            assert rejected == [1, 3] and got == want
    # below a Struct and a List: the offsets of an inner column
    inner = pa.StructArray.from_arrays([raw_list(down, child)], names=["x"])
    outer_bad = pa.ListArray.from_arrays(pa.array([0, 30, 70], type=pa.int32()), inner)
    ok_inner = pa.StructArray.from_arrays([raw_list(np.minimum(np.arange(n + 1) // 8, 10), child)], names=["x"])
    outer_ok = pa.RecordBatch.from_arrays([pa.ListArray.from_arrays(pa.array([0, 30, 70], type=pa.int32()), ok_inner)], names=["o"])
    got, _, _, rejected = gpu_write([outer_ok, pa.RecordBatch.from_arrays([outer_bad], names=["o"]), outer_ok])
    assert rejected == [1] and got == NM.write_model([outer_ok, outer_ok])[0]


@pytest.mark.parametrize("t", [pa.list_(pa.int32(), 3), pa.list_view(pa.int32()), pa.dense_union([pa.field("a", pa.int32())]),
                               pa.dictionary(pa.int32(), pa.string()), pa.run_end_encoded(pa.int32(), pa.int64()),
                               pa.map_(pa.string(), pa.decimal128(10, 2)), pa.struct([("s", pa.list_(pa.date32()))]), pa.decimal256(40, 2),
                               pa.large_list(pa.struct([("d", pa.decimal128(9, 1))]))])
def test_unsupported_types_are_named_by_their_path(t):
    with pytest.raises(OrcGpuError) as e:
        ArrowWriterBuilder(io.BytesIO(), pa.schema([("top", pa.struct([("x", t)]))]), ctx=G.ctx()).try_build()
    assert e.value.code == UNSUPPORTED and "top.x" in str(e.value)


def test_out_of_scope_row_index_and_device_batches():
    schema = pa.schema([("l", pa.list_(pa.float32())), ("i", pa.int32())])
    with pytest.raises(OrcGpuError) as e:
        ArrowWriterBuilder(io.BytesIO(), schema, ctx=G.ctx()).with_row_index_stride(100).try_build()
    assert e.value.code == UNSUPPORTED and "row index" in str(e.value)
    w = ArrowWriterBuilder(io.BytesIO(), schema, ctx=G.ctx()).try_build()
    b = pa.RecordBatch.from_arrays([pa.array([[1.0], []], type=pa.list_(pa.float32())), pa.array([1, 2], type=pa.int32())], schema=schema)
    from orc_rust_amd.arrow_writer import _ARRAY_BYTES, _Exported, _export_schema
    s, a = _export_schema(b.schema), _Exported(_ARRAY_BYTES)
    b._export_to_c(a.addr)
    try:
        with pytest.raises(OrcGpuError) as e:  # (refused before a buffer is looked at)
            w.write_c(s.addr, a.addr, capi.ENC_ON_DEVICE)
        assert e.value.code == UNSUPPORTED and "device" in str(e.value)
    finally:
        a.release()
        s.release()
    w.write(b)  # the writer stays usable
    w.close()
    w.free()
    # a schema that differs below the top level is not the writer's
    w = ArrowWriterBuilder(io.BytesIO(), schema, ctx=G.ctx()).try_build()
    other = pa.RecordBatch.from_arrays([pa.array([[1.0]], type=pa.list_(pa.float64())), pa.array([1], type=pa.int32())], names=["l", "i"])
    with pytest.raises(OrcGpuError) as e:
        w.write(other)
    assert e.value.code == UNEXPECTED
    w.free()


def _round_trips(n_lists):
    rng = np.random.default_rng(17)
    cols = [list_array(5000, rng, ints(rng, np.int32, 0.1), nulls=0.1 * (i % 2)) for i in range(n_lists)]
    b = pa.RecordBatch.from_arrays(cols, names=["c%d" % i for i in range(n_lists)])
    w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).try_build()
    w.write(b)
    w.flush_stripe()  # (the first stripe grows the buffers)
    s0 = w.stats()
    for _ in range(3):
        w.write(b)
        w.flush_stripe()
    s1 = w.stats()
    w.close()
    w.free()
    return (s1["round_trips"] - s0["round_trips"]) / 3, (s1["stripe_round_trips"] - s0["stripe_round_trips"]) / (s1["stripes"] - s0["stripes"])


def test_round_trips_do_not_grow_with_the_tree():
    """a tree of 2 columns (one List) and one of 20 (ten Lists): the same host waits per write, and two per stripe"""
    a, b = _round_trips(1), _round_trips(10)
    assert a == b, (a, b)
    assert a[1] == 2, a


@pytest.mark.parametrize("comp", [None, "snappy", "lz4"])
def test_flat_schemas_are_byte_for_byte_what_they_were(comp):
    O.lib()
    rng = np.random.default_rng(18)
    n = 3000
    b = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 50, n).astype(np.int32), mask=rng.random(n) < 0.1), strings(rng, 0.1)(n),
                                    pa.array(rng.random(n)), pa.array(rng.random(n) < 0.3), pa.array(rng.integers(-3, 3, n).astype(np.int8))],
                                   names=["i", "s", "f", "b", "c"])
    want, want_rows = WM.write_model([b, b.slice(7, 1000)], batch_size=100, stripe_byte_size=9000)
    got, rows, stats, _ = gpu_write([b, b.slice(7, 1000)], batch_size=100, sbs=9000, comp=comp, block=4096)
    assert rows == want_rows and len(rows) > 2
    assert stats["nested_gathers"] == 0 and stats["nested_slices"] == 0
    if comp:
        check_chunked(got, want, comp, 4096)
    else:
        assert got == want


@pytest.mark.parametrize("stem", ["nested_array_float", "nested_map_struct", "nested_struct"])
def test_golden_files_round_trip(stem):
    """read with ArrowReaderBuilder, written, read again: the two reads are equal (no golden leaf type is projected away: the
    three files hold lists of floats, maps of strings to structs and structs of the flat writer's types)"""
    first = list(ArrowReaderBuilder.try_new(A.data_path(stem + ".orc"), ctx=G.ctx()).build())
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, first[0].schema, ctx=G.ctx()).try_build()
    for b in first:
        w.write(b)
    w.close()
    w.free()
    again = list(ArrowReaderBuilder.try_new(out.getvalue(), ctx=G.ctx()).build())
    assert pa.Table.from_batches(again).to_pylist() == pa.Table.from_batches(first).to_pylist()
    assert po.ORCFile(io.BytesIO(out.getvalue())).read().to_pylist() == pa.Table.from_batches(first).to_pylist()
