"""Snappy and LZ4 compression on the GPU (orcgpu_compress_stream, orcgpu_writer_set_compression, ArrowWriterBuilder.with_compression).

Every compressed stream is checked against two independent decoders: the CPU oracle's ORC stream decompressor and pyarrow's own
Snappy / LZ4 block codecs, chunk by chunk.  A compressed file must be the uncompressed writer's file plus chunking: the same
stripes and rows, and every stream, decompressed, byte for byte the stream of the Python model of the reference writer."""
import ctypes as C
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import gpu_util as G
import oracle_lib as O
import orcfile
import writer_model as WM
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder, capi

pytestmark = pytest.mark.gpu

CODECS = ["snappy", "lz4"]
PA_CODEC = {"snappy": "snappy", "lz4": "lz4_raw"}
KIND = {"snappy": 2, "lz4": 4}


# ---- chunks -------------------------------------------------------------------------------------------------------------------

def split_chunks(data):
    """[(is_original, payload)] of an ORC compressed stream"""
    out, at = [], 0
    while at < len(data):
        h = data[at] | data[at + 1] << 8 | data[at + 2] << 16
        n = h >> 1
        out.append((bool(h & 1), data[at + 3:at + 3 + n]))
        at += 3 + n
    assert at == len(data)
    return out


def check_stream(comp, raw, codec, block_size):
    """comp decodes to raw with the oracle and, chunk by chunk, with pyarrow; chunks obey the size and original-chunk rules.
    Returns (payload bytes, pyarrow's compressed bytes of the same chunks under the same original-chunk rule)."""
    st, back = O.stream_decompress(comp, codec, block_size)
    assert st == 0 and back == raw, "the oracle decodes something else (%d)" % st
    chunks = split_chunks(comp)
    assert len(chunks) == (len(raw) + block_size - 1) // block_size
    ours = theirs = 0
    for k, (orig, payload) in enumerate(chunks):
        piece = raw[k * block_size:(k + 1) * block_size]
        assert len(payload) <= block_size
        if orig:
            assert payload == piece
        else:
            assert len(payload) < len(piece), "a compressed chunk that is not smaller than its input"
            got = pa.decompress(payload, decompressed_size=len(piece), codec=PA_CODEC[codec], asbytes=True)
            assert got == piece, "pyarrow decodes chunk %d to something else" % k
        ours += len(payload)
        theirs += min(len(pa.compress(piece, codec=PA_CODEC[codec], asbytes=True)), len(piece))
    return ours, theirs


def _inputs(block_size):
    rng = np.random.default_rng(block_size)
    text = b" ".join(b"the quick brown fox %d jumps over the lazy dog %s" % (i, b"x" * (i % 13)) for i in range(4000))
    block = rng.integers(0, 256, 70 * 1024, dtype=np.uint8).tobytes()
    piece = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    cross = b"".join(piece + rng.integers(0, 256, 7000 + 311 * i, dtype=np.uint8).tobytes() for i in range(12))
    return {
        "empty": b"",
        "one": b"\x07",
        "block-1": text[:block_size - 1],
        "block": text[:block_size],
        "block+1": text[:block_size + 1],
        "random": rng.integers(0, 256, 150_000, dtype=np.uint8).tobytes(),
        "zeros": bytes(200_000),
        "period3": b"abc" * 40_000,
        "period7": rng.integers(0, 256, 7, dtype=np.uint8).tobytes() * 20_000,
        "period70k": block * 3,  # (matches past 64 KiB: out of reach)
        "cross-segments": cross,
        "text": text,
    }


@pytest.mark.parametrize("block_size", [64, 1024, 65536, 262144])
@pytest.mark.parametrize("codec", CODECS)
def test_stream_against_two_decoders(codec, block_size):
    ctx = G.ctx()
    for name, raw in _inputs(block_size).items():
        comp = ctx.compress_stream(raw, codec, block_size)
        check_stream(comp, raw, codec, block_size)
        if name == "random" and block_size >= 1024:
            assert all(orig for orig, _ in split_chunks(comp)), "random bytes must come out as original chunks"
        if (name in ("zeros", "period3") and block_size >= 1024) or (name == "text" and block_size >= 65536):
            assert len(comp) < len(raw) // 2, (name, len(comp), len(raw))
        assert ctx.compress_stream(raw, codec, block_size) == comp, "two runs differ (%s)" % name


@pytest.mark.parametrize("codec", CODECS)
def test_stream_from_device_memory(codec):
    ctx = G.ctx()
    hip = C.CDLL("libamdhip64.so")
    bs = 65536
    for name, raw in _inputs(bs).items():
        if not raw:
            continue
        bound = len(raw) + 3 * ((len(raw) + bs - 1) // bs)
        d_in, d_out = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_in), C.c_size_t(len(raw))) == 0
        assert hip.hipMalloc(C.byref(d_out), C.c_size_t(bound)) == 0
        try:
            assert hip.hipMemcpy(d_in, C.c_char_p(raw), C.c_size_t(len(raw)), 1) == 0
            n = ctx.compress_stream_device(d_in, len(raw), codec, d_out, bound, bs)
            out = (C.c_uint8 * max(1, n))()
            assert hip.hipMemcpy(out, d_out, C.c_size_t(n), 2) == 0
            comp = bytes(out)[:n]
        finally:
            hip.hipFree(d_in)
            hip.hipFree(d_out)
        assert comp == ctx.compress_stream(raw, codec, bs), "device input gives other bytes than host input (%s)" % name
        check_stream(comp, raw, codec, bs)


def test_stream_errors():
    ctx = G.ctx()
    for kind in ("zstd", "zlib", "lzo"):
        with pytest.raises(capi.OrcGpuError) as e:
            ctx.compress_stream(b"abcd", kind)
        assert e.value.code == 7  # ORCGPU_UNSUPPORTED
    with pytest.raises(capi.OrcGpuError) as e:
        ctx.compress_stream(b"abcd", "snappy", 1 << 23)
    assert e.value.code == 101


# ---- the writer ---------------------------------------------------------------------------------------------------------------
# (helpers of test_gpu_writer.py, copied)

ALL_TYPES = [pa.bool_(), pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.float32(), pa.float64(), pa.string(), pa.large_string(),
             pa.binary(), pa.large_binary()]


def _column(t, n, rng, mode):
    if t == pa.bool_():
        py = (rng.random(n) < 0.3).tolist()
    elif pa.types.is_integer(t):
        bits = t.bit_width
        lo, hi = -(1 << (bits - 3)), (1 << (bits - 3))
        base = np.repeat(rng.integers(lo, hi, n // 6 + 2), rng.integers(1, 12, n // 6 + 2))[:n]
        if len(base) < n:
            base = np.concatenate([base, rng.integers(lo, hi, n - len(base))])
        base[n // 3: n // 2] = np.arange(n // 2 - n // 3) % (hi - 1)
        py = base.tolist()
    elif pa.types.is_floating(t):
        py = rng.standard_normal(n).astype(np.float32 if t == pa.float32() else np.float64).tolist()
    else:
        words = [b"", b"a", b"orc", b"\xff\x00zz", b"longer value here"]
        py = [words[i % 5] * (1 + i % 3) for i in rng.integers(0, 1000, n)]
        if pa.types.is_string(t) or pa.types.is_large_string(t):
            py = [x.decode("latin-1") for x in py]
    if mode == "plain":
        return pa.array(py, type=t)
    mask = rng.random(n) < 0.25 if mode == "nulls" else np.zeros(n, dtype=bool)
    arr = pa.array(py, type=t, mask=mask)
    if mode == "bitmap" and arr.buffers()[0] is None:
        bm = pa.py_buffer(np.packbits(np.ones(n, dtype=np.uint8), bitorder="little").tobytes())
        arr = pa.Array.from_buffers(t, n, [bm] + arr.buffers()[1:], null_count=-1)
    return arr


def _batch(n, rng, mode="nulls", types=ALL_TYPES):
    return pa.RecordBatch.from_arrays([_column(t, n, rng, mode) for t in types], names=["c%d" % i for i in range(len(types))])


def _plain_types(table):
    fields = []
    for f in table.schema:
        t = {pa.large_string(): pa.string(), pa.large_binary(): pa.binary()}.get(f.type, f.type)
        fields.append(pa.field(f.name, t))
    return table.cast(pa.schema(fields))


def check_readers(data, batches, schema=None):
    expect = _plain_types(pa.Table.from_batches(batches, schema=schema or batches[0].schema))
    got = po.ORCFile(io.BytesIO(data)).read()
    assert got.equals(expect), "pyarrow.orc read back something else"
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    assert sum(b.num_rows for b in mine) == expect.num_rows
    if expect.num_rows:
        for i, f in enumerate(expect.schema):
            got_col = pa.concat_arrays([b.column(i) for b in mine])
            assert got_col.equals(expect.column(i).combine_chunks()), "ArrowReaderBuilder read back something else in %s" % f.name


def comp_write(batches, codec, block_size=262144, schema=None, batch_size=1024, stripe_byte_size=64 << 20, flush_after=()):
    schema = schema or batches[0].schema
    out = io.BytesIO()
    b = ArrowWriterBuilder(out, schema, ctx=G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(stripe_byte_size)
    w = b.with_compression(codec, block_size).try_build()
    for i, x in enumerate(batches):
        w.write(x)
        if i in flush_after:
            w.flush_stripe()
    w.close()
    rows, stats = w.stripe_rows(), w.stats()
    w.free()
    return out.getvalue(), rows, stats


def check_chunked(got, want, codec, block_size):
    """got: a compressed file; want: the uncompressed one.  Returns (our payload bytes, pyarrow's) over every stream."""
    f, u = orcfile.OrcFile(got), orcfile.OrcFile(want)
    assert f.compression == KIND[codec] and f.block_size == block_size
    assert len(f.stripes) == len(u.stripes) and f.number_of_rows == u.number_of_rows
    ours = theirs = 0
    for sf, su in zip(f.stripes, u.stripes):
        assert sf.number_of_rows == su.number_of_rows
        assert [(k, c) for k, c, _ in sf.stream_list] == [(k, c) for k, c, _ in su.stream_list]
        assert sf.encodings == su.encodings
        for key, raw in su.streams.items():
            o, t = check_stream(sf.streams[key], raw, codec, block_size)
            ours, theirs = ours + o, theirs + t
    return ours, theirs


def check(batches, codec, block_size=262144, schema=None, flush_after=(), **kw):
    O.lib()
    want, want_rows = WM.write_model(batches, schema=schema, flush_after=flush_after, **kw)
    got, rows, stats = comp_write(batches, codec, block_size, schema=schema, flush_after=flush_after, **kw)
    assert rows == want_rows, (rows, want_rows)
    check_chunked(got, want, codec, block_size)
    check_readers(got, batches, schema)
    return rows, stats


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("mode", ["plain", "bitmap", "nulls"])
def test_every_type(codec, mode):
    rng = np.random.default_rng({"plain": 1, "bitmap": 2, "nulls": 3}[mode])
    check([_batch(2500, rng, mode)], codec)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("batch_size,sbs,block_size", [(1, 256, 262144), (7, 4096, 1024), (1024, 256, 64), (1024, 1 << 20, 262144),
                                                       (8192, 64 << 20, 65536), (8192, 4096, 262144)])
def test_batch_stripe_and_block_sizes(codec, batch_size, sbs, block_size):
    rng = np.random.default_rng(batch_size * 31 + sbs)
    n = 600 if batch_size == 1 else 3000
    types = ALL_TYPES if batch_size != 1 else [pa.int8(), pa.int64(), pa.string(), pa.bool_(), pa.float32()]
    rows, _ = check([_batch(n, rng, "nulls", types)], codec, block_size, batch_size=batch_size, stripe_byte_size=sbs)
    if sbs == 256 and batch_size < n:
        assert len(rows) > 1


@pytest.mark.parametrize("codec", CODECS)
def test_flushes_slices_and_empty_batches(codec):
    rng = np.random.default_rng(9)
    b1, b2 = _batch(700, rng, "plain"), _batch(300, rng, "plain")
    rows, _ = check([b1, b2, b2], codec, flush_after=(0, 1), batch_size=256)
    assert rows == [700, 300, 300]
    schema = b1.schema
    empty = pa.RecordBatch.from_arrays([pa.array([], type=f.type) for f in schema], schema=schema)
    b = _batch(4000, rng, "nulls")
    check([b.slice(13, 2000), empty, b.slice(1001, 1777), b.slice(3999, 1)], codec, schema=schema, batch_size=100, stripe_byte_size=4096)
    # no rows at all: the footer alone, as original chunks
    got, rows, _ = comp_write([], codec, schema=schema)
    assert rows == [] and po.ORCFile(io.BytesIO(got)).nrows == 0
    check_chunked(got, WM.write_model([], schema=schema)[0], codec, 262144)


@pytest.mark.parametrize("codec", CODECS)
def test_uncompressed_unchanged(codec):
    """None / "none": the uncompressed writer's file, byte for byte"""
    rng = np.random.default_rng(5)
    b = _batch(3000, rng, "nulls")
    want = WM.write_model([b], batch_size=512, stripe_byte_size=8192)[0]
    for c in (None, "none"):
        got, _, _ = comp_write([b], c, batch_size=512, stripe_byte_size=8192)
        assert got == want


# ---- device batches -------------------------------------------------------------------------------------------------------------

class _ArrowArray(C.Structure):
    pass


_ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                        ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)), ("children", C.POINTER(C.POINTER(_ArrowArray))),
                        ("dictionary", C.c_void_p), ("release", C.c_void_p), ("private_data", C.c_void_p)]


@pytest.mark.parametrize("codec", CODECS)
def test_device_batch_from_the_reader(codec):
    """A batch the GPU decoder produced, written compressed from its device buffers: the bytes of the host batch's file."""
    from orc_rust_amd import gen
    rng = np.random.default_rng(12)
    n = 20000
    present = (rng.random(n) > 0.15).astype(np.uint8)
    k = int(present.sum())
    vals = np.concatenate([np.repeat(rng.integers(0, 50, k // 8 + 1), 4)[: k // 2], rng.integers(-1 << 40, 1 << 40, k - k // 2)]).astype(np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}]
    streams = [(1, 0, gen.boolean(present)), (1, 1, gen.rle2(vals, signed=True))]
    res = G.gpu_decode(n, cols, streams, batch_size=8192)
    assert res.status()[0] == 0
    v = res.view(1, 0)
    host = res.batch(1, 0)
    m = v.length
    valid = np.unpackbits(np.frombuffer(host["validity"], dtype=np.uint8), bitorder="little")[:m].astype(bool) if v.validity else np.ones(m, bool)
    xs = np.frombuffer(host["values"], dtype=np.int64)[:m]
    hb = pa.RecordBatch.from_arrays([pa.array(xs, mask=~valid)], names=["x"])
    want, _, _ = comp_write([hb], codec, 4096, batch_size=1000, stripe_byte_size=2048)
    child = _ArrowArray()
    cbufs = (C.c_void_p * 2)(v.validity, v.values)
    child.length, child.null_count, child.offset, child.n_buffers, child.n_children, child.buffers = m, v.null_count, 0, 2, 0, cbufs
    root = _ArrowArray()
    rbufs = (C.c_void_p * 1)(None)
    kids = (C.POINTER(_ArrowArray) * 1)(C.pointer(child))
    root.length, root.null_count, root.offset, root.n_buffers, root.n_children, root.buffers, root.children = m, 0, 0, 1, 1, rbufs, kids
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, hb.schema, ctx=G.ctx()).with_batch_size(1000).with_stripe_byte_size(2048).with_compression(codec, 4096).try_build()
    sbuf = (C.c_uint8 * 72)()
    hb.schema._export_to_c(C.addressof(sbuf))
    try:
        w.write_c(C.addressof(sbuf), C.addressof(root), capi.ENC_ON_DEVICE)
    finally:
        rel = C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0]
        rel(C.addressof(sbuf))
    w.close()
    w.free()
    res.free()
    assert out.getvalue() == want
    check_chunked(want, WM.write_model([hb], batch_size=1000, stripe_byte_size=2048)[0], codec, 4096)
    check_readers(want, [hb])


# ---- host round trips -------------------------------------------------------------------------------------------------------------

def _round_trips_per_stripe(types, codec, sbs=64 << 20):
    rng = np.random.default_rng(14)
    b = _batch(20000, rng, "nulls", types)
    w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).with_stripe_byte_size(sbs).with_compression(codec).try_build()
    w.write(b)
    w.flush_stripe()  # (the first stripe grows the buffers)
    s0 = w.stats()
    for _ in range(3):
        w.write(b)
        w.flush_stripe()
    s1 = w.stats()
    w.close()
    w.free()
    return (s1["stripe_round_trips"] - s0["stripe_round_trips"]) / (s1["stripes"] - s0["stripes"])


@pytest.mark.parametrize("codec", CODECS)
def test_round_trips_per_stripe(codec):
    """A compressed stripe costs two host round trips, for 2 columns and for 16."""
    two = [pa.int64(), pa.string()]
    sixteen = [pa.int64(), pa.int32(), pa.int16(), pa.int8(), pa.bool_(), pa.float32(), pa.float64(), pa.string(), pa.large_string(),
               pa.binary(), pa.large_binary(), pa.int64(), pa.int32(), pa.string(), pa.int8(), pa.bool_()]
    assert _round_trips_per_stripe(two, codec) == 2
    assert _round_trips_per_stripe(sixteen, codec) == 2
    assert _round_trips_per_stripe(two, codec, 64 << 10) == _round_trips_per_stripe(sixteen, codec, 64 << 10) == 2


# ---- ratio --------------------------------------------------------------------------------------------------------------------

def _one(a):
    return a.combine_chunks() if isinstance(a, pa.ChunkedArray) else a


def _lineitem(n, rng):
    return pa.RecordBatch.from_pydict({k: _one(v) for k, v in {
        "l_orderkey": pa.array(np.repeat(np.arange(n // 4 + 1, dtype=np.int64) * 4, 4)[:n]),
        "l_partkey": pa.array(rng.integers(1, 200000, n).astype(np.int64)),
        "l_suppkey": pa.array(rng.integers(1, 10000, n).astype(np.int64)),
        "l_linenumber": pa.array((np.arange(n) % 7 + 1).astype(np.int32)),
        "l_quantity": pa.array(rng.integers(1, 51, n).astype(np.float64)),
        "l_extendedprice": pa.array(np.round(rng.random(n) * 100000, 2)),
        "l_discount": pa.array(rng.integers(0, 11, n) / 100.0),
        "l_tax": pa.array(rng.integers(0, 9, n) / 100.0),
        "l_returnflag": pa.array(np.array(["A", "N", "R"])[rng.integers(0, 3, n)]),
        "l_linestatus": pa.array(np.array(["O", "F"])[rng.integers(0, 2, n)]),
        "l_shipdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)),
        "l_commitdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)),
        "l_receiptdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)),
        "l_shipinstruct": pa.array(np.array(["DELIVER IN PERSON", "COLLECT COD", "NONE", "TAKE BACK RETURN"])[rng.integers(0, 4, n)]),
        "l_shipmode": pa.array(np.array(["AIR", "MAIL", "SHIP", "TRUCK", "RAIL", "FOB", "REG AIR"])[rng.integers(0, 7, n)]),
        "l_comment": pa.array(["c%x" % x for x in rng.integers(0, 1 << 40, n)]),
    }.items()})


# measured on the lineitem-shaped table below: payload bytes against pyarrow's compressors over the same chunks,
# and the file against the uncompressed one
RATIO_VS_PYARROW = 1.15
SMALLER_THAN_UNCOMPRESSED = {"snappy": 1.8, "lz4": 1.65}


@pytest.mark.parametrize("codec", CODECS)
def test_ratio_lineitem(codec):
    rng = np.random.default_rng(13)
    b = _lineitem(300_000, rng)
    got, rows, _ = comp_write([b], codec, stripe_byte_size=8 << 20)
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, b.schema, ctx=G.ctx()).with_stripe_byte_size(8 << 20).try_build()
    w.write(b)
    w.close()
    assert w.stripe_rows() == rows
    w.free()
    plain = out.getvalue()
    ours, theirs = check_chunked(got, plain, codec, 262144)
    print("%s: %d payload bytes, pyarrow %d (%.3fx); file %d, uncompressed %d (%.2fx smaller)" % (
        codec, ours, theirs, ours / theirs, len(got), len(plain), len(plain) / len(got)))
    assert ours <= RATIO_VS_PYARROW * theirs, (ours, theirs)
    assert len(got) * SMALLER_THAN_UNCOMPRESSED[codec] <= len(plain), (len(got), len(plain))
    assert po.ORCFile(io.BytesIO(got)).read().equals(pa.Table.from_batches([b]))


# ---- errors -------------------------------------------------------------------------------------------------------------------

def _raw_writer(schema):
    return ArrowWriterBuilder(io.BytesIO(), schema, ctx=G.ctx()).try_build()


def test_errors():
    schema = pa.schema([("x", pa.int64())])
    L = G.ctx().L
    w = _raw_writer(schema)
    for kind in (1, 3, 5):  # ZLIB, LZO, ZSTD
        assert L.orcgpu_writer_set_compression(w._h, kind, 0) == 7  # ORCGPU_UNSUPPORTED
    assert L.orcgpu_writer_set_compression(w._h, 2, 1 << 23) == 101  # past the chunk header's limit
    assert L.orcgpu_writer_set_compression(w._h, 2, (1 << 23) - 1) == 0
    assert L.orcgpu_writer_set_compression(w._h, 4, 0) == 0
    w.write(pa.RecordBatch.from_pydict({"x": pa.array([1, 2, 3], pa.int64())}))
    assert L.orcgpu_writer_set_compression(w._h, 2, 0) == 101  # after a write
    w.close()
    w.free()
    for call in ("flush_stripe", "close"):
        w = _raw_writer(schema)
        getattr(w, call)()
        assert L.orcgpu_writer_set_compression(w._h, 2, 0) == 101
        w.free()
