"""ArrowWriter with Bloom filters (orcgpu_writer_set_bloom_filter, ArrowWriterBuilder.with_bloom_filter_columns): a
BLOOM_FILTER_UTF8 stream behind the ROW_INDEX of each listed column, built on the GPU.

- the streams of the Int, String, Double and Binary columns of Apache ORC's bloom_filter.orc are reproduced byte for byte;
- at the edges (strides, nulls, slicing, stripes, every integer and float width, every Murmur3 tail) the streams are
  tests/writer_bloom_model.py's, from the LDS kernel and from the global one;
- nothing else of the file changes, and compression, dictionaries and device batches do not change the filters;
- the reader prunes with them exactly the row groups the model's test_hash rules out."""
import ctypes as C
import io
import struct

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import arrow_util as A
import gpu_util as G
import oracle_lib as O
import writer_bloom_model as BM
from orcfile import BLOOM_FILTER_UTF8, ROW_INDEX, OrcFile
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder, capi
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from test_gpu_writer import _DeviceBatch, _plain_types

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID_ARGUMENT = 7, 101  # include/orcgpu.h


def write(batches, stride, bloom=None, fpp=0.01, comp=None, block_size=None, batch_size=1024, sbs=64 << 20, flush_after=(), dictionary=0.0):
    out = io.BytesIO()
    b = ArrowWriterBuilder(out, batches[0].schema, ctx=G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(sbs)
    if comp:
        b = b.with_compression(comp, block_size) if block_size else b.with_compression(comp)
    b = b.with_row_index_stride(stride)
    if dictionary:
        b = b.with_dictionary_key_size_threshold(dictionary)
    if bloom is not None:
        b = b.with_bloom_filter_columns(bloom, fpp=fpp)
    w = b.try_build()
    for i, x in enumerate(batches):
        w.write(x)
        if i in flush_after:
            w.flush_stripe()
    w.close()
    rows, stats, counts = w.stripe_rows(), w.stats(), w.dictionary_counts()
    w.free()
    return out.getvalue(), rows, stats, counts


def index_order(stripe):
    """(kind, column) of the stripe's index streams, in file order"""
    return [(k, c) for k, c, _ in stripe.stream_list if k in (ROW_INDEX, BLOOM_FILTER_UTF8)]


def want_order(schema, bloom):
    out = [(ROW_INDEX, 0)]
    for i, name in enumerate(schema.names):
        out.append((ROW_INDEX, i + 1))
        if name in bloom:
            out.append((BLOOM_FILTER_UTF8, i + 1))
    return out


def check_streams(data, table, rows, stride, bloom, fpp):
    """every listed column's stream in every stripe against the model; the order of the index streams; index_length"""
    O.lib()
    of = OrcFile(data)
    assert [s.number_of_rows for s in of.stripes] == rows
    for s in of.stripes:
        assert index_order(s) == want_order(table.schema, bloom)
        n_index = len(index_order(s))
        assert s.index_length == sum(l for _, _, l in s.stream_list[:n_index])
    for i, name in enumerate(table.schema.names):
        got = BM.file_streams(of, i + 1)
        if name not in bloom:
            assert got == [None] * len(rows), name
            continue
        want = BM.column_streams(table.column(name), rows, stride, fpp)
        for si in range(len(rows)):
            assert got[si] == want[si], (name, si)
    return of


def other_streams(of):
    return [[(k, c, bytes(s.streams[(c, k)])) for k, c, _ in s.stream_list if k != BLOOM_FILTER_UTF8] for s in of.stripes]


def same_table(got, want):
    assert got.num_rows == want.num_rows and got.column_names == want.column_names
    for name in want.column_names:
        a, b = got.column(name).combine_chunks(), want.column(name).combine_chunks()
        assert a.is_null().equals(b.is_null()), name
        if pa.types.is_floating(b.type):  # (NaN equal to itself)
            np.testing.assert_array_equal(a.fill_null(0).to_numpy(), b.fill_null(0).to_numpy())
        else:
            assert a.equals(b), name


# ---- fixture parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", [None, "snappy"])
def test_fixture_parity(comp):
    """the four columns of Apache ORC's bloom_filter.orc the model reproduces, written with its stride and probability"""
    O.lib()
    names = ["id", "name", "score", "data"]
    table = A.expected_table("bloom_filter").select(names)
    fixture = OrcFile(A.data_path("bloom_filter.orc"))
    ids = {n: c for n, c, _ in fixture.root_columns()}
    data, rows, _, _ = write(table.combine_chunks().to_batches(), 10000, names, 0.01, comp)
    assert rows == [204]
    of = OrcFile(data)
    assert index_order(of.stripes[0]) == [(6, 0), (6, 1), (8, 1), (6, 2), (8, 2), (6, 3), (8, 3), (6, 4), (8, 4)]
    for i, n in enumerate(names):
        (got,), (want,) = BM.file_streams(of, i + 1), BM.file_streams(fixture, ids[n])
        assert got == want, n
        assert BM.filters(got)[0][0] == 7 and len(BM.filters(got)[0][1]) == 1498


# ---- model parity at the edges -------------------------------------------------------------------------------------------------
def _nan64(payload, sign=0):
    return struct.unpack("<d", struct.pack("<Q", (sign << 63) | 0x7FF0000000000000 | payload))[0]


def _edge_table(n=3000):
    rng = np.random.default_rng(41)
    quarter = rng.random(n) < 0.25

    def ints(dt):
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        a[:6] = [info.min, info.max, -1, 0, 1, info.min + 1]
        a[n - 1] = info.min
        return a

    f64 = rng.standard_normal(n)
    f64[:10] = [np.inf, -np.inf, -0.0, 0.0, _nan64(1 << 51), _nan64(1), _nan64(0x7FFFFFFFFFFFF), _nan64(1 << 51, 1), 5e-324, 1.7976931348623157e308]
    f32 = rng.standard_normal(n).astype(np.float32)
    f32[:9] = np.array([np.inf, -np.inf, -0.0, 0.0, 1e-45, 3.4028235e38, 0.1, -0.1, 1.0], dtype=np.float32)
    f32.view(np.uint32)[9:12] = [0x7FC00000, 0x7F800001, 0xFFC12345]  # NaNs of three payloads
    # strings of every length 0 .. 40 (Murmur3: 0 .. 5 blocks, tails 0 .. 7), bytes >= 0x80, a few long ones
    raw = [bytes(rng.integers(0, 256, i % 41, dtype=np.uint8)) for i in range(n)]
    for i, ln in ((50, 300), (51, 301), (1500, 1027), (2999, 333)):
        raw[i] = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
    text = ["".join(chr(0x61 + b % 26) if b < 0xC0 else "é" for b in r) for r in raw]  # (valid UTF-8, 1 and 2 byte characters)
    dead = np.zeros(n, bool)
    dead[1000:2000] = True  # (stride 1000: an all-null group; stride 7: many)
    cols = {
        "i8": pa.array(ints(np.int8)), "i16": pa.array(ints(np.int16), mask=quarter), "i32": pa.array(ints(np.int32)),
        "i64": pa.array(ints(np.int64), mask=dead),
        "f32": pa.array(f32), "f64": pa.array(f64, mask=np.roll(quarter, 12)),
        "s": pa.array(text, mask=quarter), "ls": pa.array(text[::-1], type=pa.large_string()),
        "bin": pa.array(raw, type=pa.binary()), "lbin": pa.array(raw[::-1], type=pa.large_binary(), mask=dead),
        "flag": pa.array(rng.random(n) < 0.5),  # (not listed: a column without a filter in between)
    }
    return pa.RecordBatch.from_pydict(cols)


EDGE = None


def edge_batch():
    global EDGE
    if EDGE is None:
        EDGE = _edge_table()
    return EDGE


@pytest.mark.parametrize("stride", [1, 7, 1000, 5000])
def test_model_parity_at_the_edges(stride):
    """batches of 7 rows, sliced batches with offsets, an empty batch between writes, three stripes, a short last group, an
    all-null group, a stride larger than the stripe"""
    b = edge_batch()
    bloom = [n for n in b.schema.names if n != "flag"]
    batches = [b.slice(0, 1234), b.slice(1234, 0), b.slice(1234, 1000), b.slice(2234)]  # (offsets 1234 and 2234 inside the arrays)
    data, rows, _, _ = write(batches, stride, bloom, 0.01, batch_size=7, flush_after=(0, 2))
    assert rows == [1234, 1000, 766]
    check_streams(data, pa.Table.from_batches(batches), rows, stride, bloom, 0.01)


@pytest.mark.parametrize("stride,fpp,n", [(50000, 0.001, 60000), (10000, 0.01, 25000)])
def test_both_bitset_paths(stride, fpp, n):
    """a bitset of about 90 KB (built in global memory) and one of 12 KB (built in LDS)"""
    words, _ = BM.size(stride, fpp)
    assert (words * 8 > 48 << 10) == (stride == 50000)
    rng = np.random.default_rng(stride)
    b = pa.RecordBatch.from_pydict({
        "k": pa.array(rng.integers(-1 << 62, 1 << 62, n), mask=rng.random(n) < 0.1),
        "s": pa.array(["c%x" % x for x in rng.integers(0, 1 << 40, n)]),
    })
    data, rows, _, _ = write([b], stride, ["k", "s"], fpp)
    assert rows == [n]
    check_streams(data, pa.Table.from_batches([b]), rows, stride, ["k", "s"], fpp)


# ---- everything else unchanged -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", [None, "lz4"])
def test_nothing_else_changes(comp):
    b = edge_batch()
    bloom = ["i64", "f32", "s", "lbin"]
    batches = [b.slice(0, 1700), b.slice(1700)]
    base, rows0, _, _ = write(batches, 1000, None, comp=comp, batch_size=333, flush_after=(0,))
    data, rows, _, _ = write(batches, 1000, bloom, comp=comp, batch_size=333, flush_after=(0,))
    none, _, _, _ = write(batches, 1000, [], comp=comp, batch_size=333, flush_after=(0,))
    again, _, _, _ = write(batches, 1000, bloom, comp=comp, batch_size=333, flush_after=(0,))
    assert none == base and again == data and rows == rows0 == [1700, 1300]
    table = pa.Table.from_batches(batches)
    of = check_streams(data, table, rows, 1000, bloom, 0.01)
    assert other_streams(of) == other_streams(OrcFile(base))
    want = _plain_types(table)
    same_table(po.ORCFile(io.BytesIO(data)).read(), want)
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    same_table(pa.table({n: pa.concat_arrays([x.column(i) for x in mine]) for i, n in enumerate(want.column_names)}), want)


def test_snappy_small_blocks():
    """block_size 1024: a stream of 2 filters of 2400 bytes goes out in several chunks, and decodes to the model's bytes"""
    b = edge_batch()
    data, rows, _, _ = write([b], 2000, ["i32", "bin"], 0.01, comp="snappy", block_size=1024)
    of = check_streams(data, pa.Table.from_batches([b]), rows, 2000, ["i32", "bin"], 0.01)
    raw = of.stripes[0].streams[(3, BLOOM_FILTER_UTF8)]
    plain = BM.plain(of, raw)
    chunks, at = 0, 0
    while at < len(raw):
        h = raw[at] | raw[at + 1] << 8 | raw[at + 2] << 16
        assert h >> 1 <= 1024
        at += 3 + (h >> 1)
        chunks += 1
    assert at == len(raw) and chunks == (len(plain) + 1023) // 1024 and chunks > 2


def test_dictionary_does_not_change_the_filters():
    rng = np.random.default_rng(43)
    n = 6000
    b = pa.RecordBatch.from_pydict({"s": pa.array(["v%d" % x for x in rng.integers(0, 50, n)], mask=rng.random(n) < 0.2),
                                    "u": pa.array(["u%d" % i for i in range(n)])})
    direct, rows, _, c0 = write([b], 1000, ["s", "u"])
    data, rows1, _, c1 = write([b], 1000, ["s", "u"], dictionary=0.8)
    assert rows == rows1 and c0 == {"dictionary": 0, "direct": 2} and c1 == {"dictionary": 1, "direct": 1}
    of = check_streams(data, pa.Table.from_batches([b]), rows, 1000, ["s", "u"], 0.01)
    for cid in (1, 2):
        assert BM.file_streams(of, cid) == BM.file_streams(OrcFile(direct), cid)


def test_device_batches():
    """ORCGPU_ENC_ON_DEVICE: the same file as from the host batches"""
    b = edge_batch()
    bloom = ["i16", "f64", "s", "ls", "bin"]
    batches = [b.slice(3, 1500), b.slice(1777, 1000)]
    want, rows, _, _ = write(batches, 700, bloom, batch_size=300, flush_after=(0,))
    dev = [_DeviceBatch(x) for x in batches]
    out = io.BytesIO()
    w = (ArrowWriterBuilder(out, b.schema, ctx=G.ctx()).with_batch_size(300).with_row_index_stride(700)
         .with_bloom_filter_columns(bloom, fpp=0.01).try_build())
    sbuf = (C.c_uint8 * 72)()
    b.schema._export_to_c(C.addressof(sbuf))
    try:
        for i, d in enumerate(dev):
            w.write_c(C.addressof(sbuf), C.addressof(d.root), capi.ENC_ON_DEVICE)
            if i == 0:
                w.flush_stripe()
    finally:
        C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0](C.addressof(sbuf))
    w.close()
    w.free()
    for d in dev:
        d.free()
    assert out.getvalue() == want
    check_streams(want, pa.Table.from_batches(batches), rows, 700, bloom, 0.01)


# ---- end to end through the reader ---------------------------------------------------------------------------------------------
def _kept(data, pred):
    r = ArrowReaderBuilder.try_new(data, G.ctx()).with_predicate(pred).build()
    out = list(r)
    groups = r.row_groups()
    r.close()
    return out, groups


@pytest.mark.parametrize("kind", ["int", "string"])
def test_reader_prunes_what_the_model_says(kind):
    """every group's minimum and maximum span the probes, so only the filters can prune: eq(absent value) keeps exactly the
    groups whose filter passes the model's test_hash -- the bitsets are the model's, so the false positives are too"""
    rng = np.random.default_rng(44)
    n, S = 8000, 2000
    evens = rng.permutation(n) * 2  # even numbers 0 .. 2n - 2, every group from near 0 to near 2n
    if kind == "int":
        col, value, hash_of = pa.array(evens.astype(np.int64)), V.Int64, BM.PM.hash_long
        as_value = int
    else:
        col, value, hash_of = pa.array(["%05d" % x for x in evens]), V.Utf8, lambda s: BM.PM.murmur3_64(s.encode())
        as_value = lambda x: "%05d" % x
    b = pa.RecordBatch.from_pydict({"c": col, "row": pa.array(np.arange(n, dtype=np.int32))})
    data, rows, _, _ = write([b], S, ["c"], 0.01)
    of = check_streams(data, pa.Table.from_batches([b]), rows, S, ["c"], 0.01)
    (stream,) = BM.file_streams(of, 1)
    filts = BM.filters(stream)
    assert len(filts) == n // S
    lo, hi = evens.reshape(-1, S).min(axis=1), evens.reshape(-1, S).max(axis=1)
    probes = [int(x) for x in rng.choice(np.arange(int(lo.max()) + 1, int(hi.min()), 2), 200, replace=False)]  # odd, inside every group's range
    assert all(p % 2 == 1 for p in probes)
    pruned_all = 0
    for p in probes:
        want = [g for g in range(n // S) if BM.might_contain(filts[g], hash_of(as_value(p)))]
        out, groups = _kept(data, P.eq("c", value(as_value(p))))
        assert groups == (len(want), n // S), (p, groups, want)
        assert [int(x) for bt in out for x in bt.column(1).to_pylist()] == [r for g in want for r in range(g * S, (g + 1) * S)]
        pruned_all += not want
    assert pruned_all > 100  # (0.01 a filter, 4 filters: about 4 probes in 100 keep a group)
    for at in (0, S - 1, S, 3 * S + 17, n - 1):  # present values keep their group
        v = int(evens[at])
        want = [g for g in range(n // S) if BM.might_contain(filts[g], hash_of(as_value(v)))]
        assert at // S in want
        out, groups = _kept(data, P.eq("c", value(as_value(v))))
        assert groups == (len(want), n // S)
        assert at in [int(x) for bt in out for x in bt.column(1).to_pylist()]


# ---- round trips ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("listed", [2, 8])
def test_round_trips_unchanged(listed):
    rng = np.random.default_rng(45)
    n = 20000
    types = [np.int64, np.int32, np.int16, np.int8, np.float32, np.float64]
    cols = {"c%d" % i: pa.array(rng.integers(-100, 100, n).astype(t)) for i, t in enumerate(types)}
    cols["c6"] = pa.array(["s%d" % x for x in rng.integers(0, 1000, n)])
    cols["c7"] = pa.array([b"b%d" % x for x in rng.integers(0, 1000, n)], type=pa.binary())
    b = pa.RecordBatch.from_pydict(cols)

    def trips(bloom):
        bld = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).with_row_index_stride(3000)
        if bloom:
            bld = bld.with_bloom_filter_columns(bloom, fpp=0.01)
        w = bld.try_build()
        w.write(b)
        w.flush_stripe()
        s0 = w.stats()
        for _ in range(3):
            w.write(b)
            w.flush_stripe()
        s1 = w.stats()
        w.close()
        w.free()
        return (s1["stripe_round_trips"] - s0["stripe_round_trips"]) / 3, (s1["round_trips"] - s0["round_trips"]) / 3

    assert trips(b.schema.names[:listed]) == trips(None)
    assert trips(None)[0] == 2


# ---- errors --------------------------------------------------------------------------------------------------------------------
def _names(*names):
    return (C.c_char_p * len(names))(*[x.encode() for x in names]), len(names)


def test_errors():
    schema = pa.schema([("k", pa.int64()), ("s", pa.string()), ("flag", pa.bool_()), ("ts", pa.timestamp("us")), ("dec", pa.decimal128(10, 2)),
                        ("f", pa.float32())])
    ctx = G.ctx()
    L = ctx.L
    w = ArrowWriterBuilder(io.BytesIO(), schema, ctx=ctx).try_build()
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k"), 0.01) == INVALID_ARGUMENT  # no stride yet
    assert L.orcgpu_writer_set_row_index(w._h, 1000) == 0
    for fpp in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k"), fpp) == INVALID_ARGUMENT
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k", "nope"), 0.01) == INVALID_ARGUMENT
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k", "s", "k"), 0.01) == INVALID_ARGUMENT
    assert L.orcgpu_writer_set_bloom_filter(w._h, None, 1, 0.01) == INVALID_ARGUMENT
    for bad in ("flag", "ts", "dec"):
        assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k", bad), 0.01) == UNSUPPORTED
        assert ("'%s'" % bad) in ctx.error()
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k", "s", "f"), 0.01) == 0
    assert L.orcgpu_writer_set_row_index(w._h, 500) == INVALID_ARGUMENT  # the filters are sized from the stride
    assert L.orcgpu_writer_set_bloom_filter(w._h, None, 0, 0.01) == 0  # none again
    assert L.orcgpu_writer_set_row_index(w._h, 500) == 0
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("f"), 0.01) == 0
    b = pa.RecordBatch.from_pydict({"k": pa.array([1], pa.int64()), "s": pa.array(["a"]), "flag": pa.array([True]),
                                    "ts": pa.array([1], pa.timestamp("us")), "dec": pa.array([None], pa.decimal128(10, 2)),
                                    "f": pa.array([1.5], pa.float32())}, schema=schema)
    w.write(b)
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k"), 0.01) == INVALID_ARGUMENT  # as set_compression after a write
    w.close()
    assert L.orcgpu_writer_set_bloom_filter(w._h, *_names("k"), 0.01) == INVALID_ARGUMENT
    w.free()
    # the builder: the C call's refusal surfaces as the library's error
    with pytest.raises(Exception):
        ArrowWriterBuilder(io.BytesIO(), schema, ctx=ctx).with_row_index_stride(10).with_bloom_filter_columns(["flag"]).try_build()
